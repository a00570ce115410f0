"""rt_reproject_moving without a device: the export, the descriptor's layout against the header, the argument checks that run
before any HIP call, the binding's ValueErrors -- and properties of the restatement itself (tests/reproject_moving_expect.py), so
that the GPU parity test (tests/test_reproject_moving.py) cannot agree with a wrong one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reproject_expect as rx
import reproject_moving_expect as mx
import scene_gen as sg

RT_ERR_INVALID, RT_ERR_NO_DEVICE = 1, 2
FAKE = 0x100000   # never dereferenced: no check looks at what a pointer points to
CAMERAS = [((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 1.5, 0.1, 10.0), ((0.3, 2.2, 9.1), (0.0, 0.4, 0.0), 40.0, 48 / 32, 0.0, 9.0)]


def _same(got, want):
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def test_entry_point_is_declared_listed_and_exported(art):
    header = open(os.path.join(art.REPO_ROOT, "include", "rt_abi.h")).read()
    assert "rt_status rt_reproject_moving(const rt_reproject_desc* d, const rt_reproject_motion_desc* m," in header
    assert "rt_reproject_moving" in art.RT_ABI_SYMBOLS
    assert hasattr(art.rt_lib(), "rt_reproject_moving")
    assert art.SPHERE_DTYPE == mx.SPHERE_DTYPE and art.MEDIUM_DTYPE == mx.MEDIUM_DTYPE


def test_motion_desc_layout_matches_header(art, tmp_path):
    """sizeof and every field offset of rt_reproject_motion_desc as a C compiler lays out include/rt_abi.h."""
    fields = [f for f, _ in art.RtReprojectMotionDesc._fields_]
    assert fields == ["n_spheres", "n_media", "spheres", "prev_spheres", "media", "time", "prev_time"]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(rt_reproject_motion_desc));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof(rt_reproject_motion_desc, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(art.REPO_ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(art.RtReprojectMotionDesc)
    assert got[1:] == [getattr(art.RtReprojectMotionDesc, f).offset for f in fields]


# ------------------------------------------------------------------------------------------------- the argument checks
def _desc(art, history=True, **kw):
    d = art.RtReprojectDesc()
    d.nx, d.ny = 37, 29
    d.cur, d.prev = sg.make_camera(*CAMERAS[1], 0.0, 0.0), sg.make_camera(*CAMERAS[0], 0.0, 0.0)
    names = ["color", "depth", "alpha", "out", "out_len", "prim", "prev_prim"] + (["history", "history_len", "prev_depth", "prev_alpha"] if history else [])
    for k, name in enumerate(names):
        setattr(d, name, FAKE * (k + 1))
    d.alpha_min, d.depth_tol, d.normal_min, d.max_history = 0.5, 0.05, 0.5, 32.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _motion(art, **kw):
    m = art.RtReprojectMotionDesc()
    m.n_spheres, m.n_media, m.spheres, m.prev_spheres, m.media, m.time, m.prev_time = 10, 6, FAKE * 20, FAKE * 21, FAKE * 22, 0.5, 0.25
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_checks_name_what_failed(art):
    """Everything rt_reproject refuses and every refusal of the motion description: RT_ERR_INVALID with a text of its own that
    starts with the entry's name; a description that passes every check ends, in a process that has initialised no device, at
    RT_ERR_NO_DEVICE: the checks come before any HIP call."""
    L = art.rt_lib()
    inf, nan = float("inf"), float("nan")
    singular = sg.make_camera(*CAMERAS[0], 0.0, 0.0)
    singular.vertical[:] = singular.horizontal[:]
    good_m = _motion(art)
    cases = {
        # rt_reproject's
        "null d": (None, good_m), "nx = 0": (_desc(art, nx=0), good_m), "2^32 pixels": (_desc(art, nx=1 << 16, ny=1 << 16), good_m),
        "alpha_min = 0": (_desc(art, alpha_min=0.0), good_m), "depth_tol nan": (_desc(art, depth_tol=nan), good_m),
        "normal_min > 1": (_desc(art, normal_min=2.0), good_m), "max_history inf": (_desc(art, max_history=inf), good_m),
        "null color": (_desc(art, color=None), good_m), "null depth": (_desc(art, depth=None), good_m), "null alpha": (_desc(art, alpha=None), good_m),
        "null out": (_desc(art, out=None), good_m), "null out_len": (_desc(art, out_len=None), good_m),
        "history without len": (_desc(art, history_len=None), good_m), "len without history": (_desc(art, history=False, history_len=FAKE * 12), good_m),
        "singular prev": (_desc(art, prev=singular), good_m), "out is color": (_desc(art, out=FAKE), good_m),
        "motion overlaps out": (_desc(art, motion=FAKE * 4 + 128), good_m),
        # its own
        "null m": (_desc(art), None), "null prim": (_desc(art, prim=None), good_m), "null prev_prim": (_desc(art, prev_prim=None), good_m),
        "n_spheres < 0": (_desc(art), _motion(art, n_spheres=-1)), "n_media < 0": (_desc(art), _motion(art, n_media=-3)),
        "null spheres": (_desc(art), _motion(art, spheres=None)), "null prev_spheres": (_desc(art), _motion(art, prev_spheres=None)),
        "null media": (_desc(art), _motion(art, media=None)),
        "2^28 spheres": (_desc(art), _motion(art, n_spheres=1 << 28)), "2^28 media": (_desc(art), _motion(art, n_media=1 << 28)),
        "time nan": (_desc(art), _motion(art, time=nan)), "prev_time inf": (_desc(art), _motion(art, prev_time=-inf)),
        "out overlaps spheres": (_desc(art, out=FAKE * 20 + 32), good_m), "out_len is prev_spheres": (_desc(art, out_len=FAKE * 21), good_m),
        "motion overlaps media": (_desc(art, motion=FAKE * 22 + 8), good_m),
    }
    texts = {}
    for name, (d, m) in cases.items():
        for on_device in (0, 1):
            st = L.rt_reproject_moving(None if d is None else C.byref(d), None if m is None else C.byref(m), on_device, None, 1)
            text = L.rt_last_error_detail().decode()
            assert st == RT_ERR_INVALID and text.startswith("rt_reproject_moving"), (name, on_device, st, text)
        texts[name] = text
    same = [("null prim", "null prev_prim"), ("n_spheres < 0", "n_media < 0"), ("null spheres", "null prev_spheres"), ("2^28 spheres", "2^28 media"),
            ("time nan", "prev_time inf")]
    for group in same:
        assert len({texts[k] for k in group}) == 1, group
    distinct = [g[0] for g in same] + ["null d", "nx = 0", "2^32 pixels", "alpha_min = 0", "depth_tol nan", "normal_min > 1", "max_history inf", "null color",
                                       "null depth", "null alpha", "null out", "null out_len", "history without len", "len without history",
                                       "singular prev", "out is color", "motion overlaps out", "null m", "null media", "out overlaps spheres",
                                       "out_len is prev_spheres", "motion overlaps media"]
    assert len({texts[k] for k in distinct}) == len(distinct), texts
    for name, table in (("out overlaps spheres", "spheres"), ("out_len is prev_spheres", "prev_spheres"), ("motion overlaps media", "media")):
        assert "overlaps " + table in texts[name], (name, texts[name])
    assert "prim" in texts["null prim"] and "2^28" in texts["2^28 spheres"] and "finite" in texts["time nan"] and "media" in texts["null media"]
    # what passes: empty tables (null or not), no media, no history, every guide
    good = [(_desc(art), good_m), (_desc(art), _motion(art, n_spheres=0, spheres=None, prev_spheres=None, n_media=0, media=None)),
            (_desc(art), _motion(art, n_spheres=0, n_media=0)), (_desc(art), _motion(art, n_media=0, media=None)),
            (_desc(art, history=False), good_m), (_desc(art, normal=FAKE * 14, prev_normal=FAKE * 15, motion=FAKE * 16), good_m),
            (_desc(art), _motion(art, n_spheres=(1 << 28) - 1, spheres=FAKE * 4096, prev_spheres=FAKE * 16384, media=FAKE * 40000))]
    for k, (d, m) in enumerate(good):
        if art._initialised_device is None:
            for on_device in (0, 1):
                st = L.rt_reproject_moving(C.byref(d), C.byref(m), on_device, None, 1)
                assert st == RT_ERR_NO_DEVICE, (k, on_device, st, L.rt_last_error_detail().decode())
        else:
            st = L.rt_reproject_moving(C.byref(d), C.byref(m), 1, None, 1)
            assert st == RT_ERR_INVALID and "device memory" in L.rt_last_error_detail().decode(), (k, st)
    assert 37 * 29 * 12 < FAKE and 10 * 32 < FAKE


def test_binding_rejects_malformed_tables_before_any_device_work(art):
    c, z, ids = np.zeros((6, 8, 3), np.float32), np.zeros((6, 8), np.float32), np.zeros((6, 8), np.int32)
    cam = sg.make_camera(*CAMERAS[1], 0.0, 0.0)
    hist = dict(history=c, history_len=z, prev_depth=z, prev_alpha=z)
    sph, med = np.zeros(3, art.SPHERE_DTYPE), np.zeros(2, art.MEDIUM_DTYPE)
    bad = [
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, prev_prim=ids, prev_spheres=sph, **hist),                   # tables need spheres
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, prev_prim=ids, media=med, **hist),
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, prev_prim=ids, time=0.5, **hist),
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, prev_prim=ids, spheres=sph, **hist),                        # no prev_spheres
        lambda: art.reproject(c, z, z, cam, cam, spheres=sph, prev_spheres=sph, **hist),                               # no ids
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, spheres=sph, prev_spheres=sph, **hist),
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, prev_prim=ids, spheres=sph, prev_spheres=sph[:2], **hist),  # differing counts
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, prev_prim=ids, spheres=sph, prev_spheres=med, **hist),      # the wrong dtype
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, prev_prim=ids, spheres=np.zeros((3, 8), np.float32), prev_spheres=sph, **hist),
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, prev_prim=ids, spheres=sph, prev_spheres=sph, media=sph, **hist),
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, prev_prim=ids, spheres=[1, 2], prev_spheres=sph, **hist),   # mixed kinds
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, prev_prim=ids, spheres=sph, prev_spheres=sph, time=float("nan"), **hist),
        lambda: art.reproject(c, z, z, cam, cam, prim=ids, prev_prim=ids, spheres=sph, prev_spheres=sph, prev_time=float("inf"), **hist),
        lambda: art.TemporalAccumulator(None, art.RtFrameDesc(), follow_spheres=True),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")


# ------------------------------------------------------------------------------------------------- the restatement itself
def test_no_moved_record_is_the_static_restatement_bit_for_bit():
    """With no table, with empty tables and with tables in which no record moved, on rx.synthetic(37, 29, 7) as it is and on the
    ids of the parity test: rx.reproject's bits for every camera there."""
    s = rx.synthetic(37, 29, 7)
    painted = mx.synthetic_moving(37, 29, 7)["buffers"]
    spheres, prev_spheres, media, time, prev_time = mx.unmoved_tables()
    empty = np.zeros(0, mx.SPHERE_DTYPE)
    for b in (s["buffers"], painted):
        for name, prev in s["cams"].items():
            want = rx.reproject(cur=s["cur"], prev=prev, **b)
            for what, tables in (("none", {}), ("empty", dict(spheres=empty, prev_spheres=empty, media=media)),
                                 ("unmoved", dict(spheres=spheres, prev_spheres=prev_spheres, media=media, time=time, prev_time=prev_time))):
                details = {}
                got = mx.reproject(cur=s["cur"], prev=prev, details=details, **b, **tables)
                assert not details["followed"].any()
                for g, w, part in zip(got, want, ("out", "out_len", "motion")):
                    assert g.dtype == np.float32 and _same(g, w), (name, what, part)
    # (the ids of rx.synthetic are 0..2: with the unmoved tables they do name spheres, which then take the static path)
    assert (mx.followed_sphere(s["buffers"]["prim"], len(spheres), media) >= 0).any()


def test_synthetic_inputs_reach_every_branch():
    """The GPU test's inputs: each rule of the tail decides some pixel, and following changes what a pixel finds."""
    s = mx.synthetic_moving(37, 29, 7)
    b, t = s["buffers"], s["tables"]
    pal = mx.id_palette()
    for frame in (b["prim"], b["prev_prim"]):
        assert set(np.unique(frame)) == set(pal.tolist())
    surface = b["alpha"] >= 0.5
    k = mx.followed_sphere(b["prim"], mx.N_SPHERES, t["media"])
    assert set(np.unique(k[surface])) == set(range(-1, mx.N_SPHERES))
    in_medium = (b["prim"] >= 0) & ((b["prim"] >> 28) == mx.MEDIUM)
    assert (k[in_medium] == 0).any() and (k[in_medium] == -1).any() and (k[~surface] >= 0).any()
    sph, prev = t["spheres"], t["prev_spheres"]
    assert prev["radius"][3] == 0 and sph["radius"][4] == 0 and sph["radius"][5] < 0 and np.isnan(sph["c0"][6]).any()
    assert np.isinf(sph["vel"][7]).any() and (sph["vel"][8] != 0).any() and sph[8] == prev[8] and t["time"] != t["prev_time"]
    details = {}
    near = mx.reproject(cur=s["cur"], prev=s["cams"]["near"], details=details, **b, **t)
    static = rx.reproject(cur=s["cur"], prev=s["cams"]["near"], **b)
    f = details["followed"]
    by_sphere = np.bincount(k[f], minlength=mx.N_SPHERES)
    assert by_sphere[1] == 0 and (np.delete(by_sphere, 1) > 0).all(), by_sphere          # every record but the unmoved one is followed
    assert not f[~surface].any() and (f & in_medium).any()
    assert ((near[1] > 1) & f).sum() >= 50 and ((near[1] == 1) & f).sum() >= 50
    assert _same(near[0][~f], static[0][~f]) and _same(near[2][~f], static[2][~f])       # static pixels keep rt_reproject's bits
    assert (near[2][f] != static[2][f]).any(axis=-1).mean() > 0.9                        # ... and followed ones another motion
    for dead in (3, 4, 6, 7):                                                            # a degenerate carry ends with no history
        assert (near[1][f & (k == dead)] == 1).all(), dead
    assert (near[2][f & (k == 6)] == 0).all()                                            # a NaN centre: a is a NaN, nothing is projected
    behind = mx.reproject(cur=s["cur"], prev=s["cams"]["behind"], **b, **t)
    assert (behind[1][surface] == 1).all()
    first = mx.reproject(cur=s["cur"], prev=s["cams"]["near"], **mx.select(b, True, history=False), **t)
    assert _same(first[0], b["color"]) and (first[1] == 1).all() and _same(first[2], near[2])


def _one_sphere(nx, ny):
    """A sphere alone in front of a pinhole camera: its current record, its previous one, and the analytic depth and alpha of
    the current frame (the smaller root of |O + t dir - c|^2 = r^2 along each pixel's centre ray, in float64)."""
    cur = sg.make_camera((0.2, 0.1, 5.0), (0.0, 0.0, 0.0), 40.0, nx / ny, 0.0, 1.0, 0.0, 0.0)
    prev = sg.make_camera((0.45, 0.05, 4.9), (0.0, 0.0, 0.0), 40.0, nx / ny, 0.0, 1.0, 0.0, 0.0)
    sph = np.zeros(1, mx.SPHERE_DTYPE)
    sph["c0"], sph["radius"] = np.array([0.1, -0.05, 0.3], np.float32), 1.2
    before = sph.copy()
    before["c0"] += np.array([-0.4, 0.25, 0.15], np.float32)
    before["radius"] = 0.9
    O, LL, H, V = (np.array(list(v), np.float64) for v in (cur.origin, cur.lower_left_corner, cur.horizontal, cur.vertical))
    s = ((np.arange(nx, dtype=np.float32) + np.float32(0.5)) / np.float32(nx)).astype(np.float64)[None, :, None]
    t = ((np.arange(ny, dtype=np.float32) + np.float32(0.5)) / np.float32(ny)).astype(np.float64)[:, None, None]
    d = LL + s * H + t * V - O
    oc = O - sph["c0"][0].astype(np.float64)
    A, B, Cq = (d * d).sum(-1), (d * oc).sum(-1), (oc * oc).sum() - float(sph["radius"][0]) ** 2
    disc = B * B - A * Cq
    hit = disc > 0
    root = np.where(hit, (-B - np.sqrt(np.where(hit, disc, 0.0))) / A, 0.0)
    return dict(cur=cur, prev=prev, sph=sph, before=before, hit=hit, depth=root.astype(np.float32), alpha=hit.astype(np.float32), dir=d)


def test_motion_of_a_translated_and_grown_sphere():
    """One sphere that moved by (0.4, -0.25, -0.15) and grew from 0.9 to 1.2 under a camera that moved as well: at every pixel
    on the sphere the restatement's motion equals the projection of the carried point c' + (P - c) r' / r into the previous
    camera, evaluated in float64 from the same float32 inputs.  The bound is 4 x the largest difference measured on the CPU at
    64 x 48, 1.151e-05 pixel (float32 rounding of three dot products and two divisions scales with the frame width)."""
    nx, ny = 64, 48
    c = _one_sphere(nx, ny)
    hit = c["hit"]
    assert hit.sum() > 300 and not hit.all()
    ids = np.where(hit, mx.ref(mx.SPHERE, 0), -1).astype(np.int32)
    color = np.zeros((ny, nx, 3), np.float32)
    details = {}
    _, _, motion = mx.reproject(color, c["depth"], c["alpha"], c["cur"], c["prev"], prim=ids, prev_prim=ids, spheres=c["sph"],
                                prev_spheres=c["before"], details=details)
    assert np.array_equal(details["followed"], hit)
    O, Op, LLp, Hp, Vp = (np.array(list(v), np.float64) for v in (c["cur"].origin, c["prev"].origin, c["prev"].lower_left_corner,
                                                                  c["prev"].horizontal, c["prev"].vertical))
    P = O + c["depth"].astype(np.float64)[..., None] * c["dir"]
    cc, cp = c["sph"]["c0"][0].astype(np.float64), c["before"]["c0"][0].astype(np.float64)
    carried = cp + (P - cc) * (float(c["before"]["radius"][0]) / float(c["sph"]["radius"][0]))
    basis = np.stack([LLp - Op, Hp, Vp], axis=1)                        # q = a (A + s H + t V)
    ast = np.linalg.solve(basis, (carried - Op).reshape(-1, 3).T).T.reshape(ny, nx, 3)
    assert (ast[hit][:, 0] > 0).all()
    want = np.stack([ast[..., 1] / ast[..., 0] * nx - 0.5 - np.arange(nx)[None, :], ast[..., 2] / ast[..., 0] * ny - 0.5 - np.arange(ny)[:, None]], axis=-1)
    worst = float(np.abs(motion.astype(np.float64) - want)[hit].max())
    print(f"largest |motion - float64 projection| on the sphere: {worst:.3e} pixel")
    assert np.abs(want[hit]).max() > 3.0                                # whole pixels, not a rounding matter
    assert worst <= 4 * 1.151e-05
    # without following the same pixels report the camera's motion only, which is another one
    static = rx.reproject(color, c["depth"], c["alpha"], c["cur"], c["prev"])[2]
    assert np.linalg.norm(static.astype(np.float64) - want, axis=-1)[hit].min() > 0.5
    assert np.array_equal(static[~hit], motion[~hit])                   # sky never follows
