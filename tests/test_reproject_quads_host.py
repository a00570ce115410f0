"""rt_reproject_quads without a device: the export, the descriptor's layout against the header, the argument checks that run before
any HIP call, the binding's ValueErrors -- and properties of the restatement itself (tests/reproject_quads_expect.py), so that the
GPU parity test (tests/test_reproject_quads.py) cannot agree with a wrong one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reproject_instances_expect as ix
import reproject_quads_expect as qx
import scene_gen as sg

RT_ERR_INVALID, RT_ERR_NO_DEVICE = 1, 2
FAKE = 0x100000   # never dereferenced: no check looks at what a pointer points to
CAMERAS = [((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 1.5, 0.1, 10.0), ((0.3, 2.2, 9.1), (0.0, 0.4, 0.0), 40.0, 48 / 32, 0.0, 9.0)]
U = 2.0 ** -24    # the unit roundoff of binary32


def _same(got, want):
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def test_entry_point_is_declared_listed_and_exported(art):
    header = open(os.path.join(art.REPO_ROOT, "include", "rt_abi.h")).read()
    assert ("rt_status rt_reproject_quads(const rt_reproject_desc* d, const rt_reproject_motion_desc* m,\n"
            "                             const rt_reproject_instance_desc* im, const rt_reproject_quad_desc* qm,\n"
            "                             int buffers_on_device, void* stream, int blocking);") in header
    assert "rt_reproject_quads" in art.RT_ABI_SYMBOLS
    assert hasattr(art.rt_lib(), "rt_reproject_quads")
    assert art.QUAD_DTYPE == qx.QUAD_DTYPE and art.QUAD_DTYPE.itemsize == 80
    assert art.RT_PRIM_QUAD == qx.QUAD


def test_quad_desc_layout_matches_header(art, tmp_path):
    """sizeof (24 bytes) and every field offset of rt_reproject_quad_desc as a C compiler lays out include/rt_abi.h."""
    fields = [f for f, _ in art.RtReprojectQuadDesc._fields_]
    assert fields == ["n_quads", "reserved", "quads", "prev_quads"]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(rt_reproject_quad_desc));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof(rt_reproject_quad_desc, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(art.REPO_ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(art.RtReprojectQuadDesc) == 24
    assert got[1:] == [getattr(art.RtReprojectQuadDesc, f).offset for f in fields]


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


def _instances(art, history=True, **kw):
    im = art.RtReprojectInstanceDesc()
    im.n_instances, im.instances, im.prev_instances, im.inst = 12, FAKE * 30, FAKE * 31, FAKE * 32
    im.prev_inst = FAKE * 33 if history else None
    for k, v in kw.items():
        setattr(im, k, v)
    return im


def _quads(art, **kw):
    qm = art.RtReprojectQuadDesc()
    qm.n_quads, qm.quads, qm.prev_quads = 10, FAKE * 40, FAKE * 41
    for k, v in kw.items():
        setattr(qm, k, v)
    return qm


def test_checks_name_what_failed(art):
    """Everything rt_reproject_instances refuses and every refusal of the quad description: RT_ERR_INVALID with a text of its own
    that starts with the entry's name, on both buffers_on_device values; a description that passes every check ends, in a process
    that has initialised no device, at RT_ERR_NO_DEVICE: the checks come before any HIP call."""
    L = art.rt_lib()
    inf, nan = float("inf"), float("nan")
    singular = sg.make_camera(*CAMERAS[0], 0.0, 0.0)
    singular.vertical[:] = singular.horizontal[:]
    gm, gi, gq = _motion(art), _instances(art), _quads(art)
    cases = {
        # rt_reproject's
        "null d": (None, gm, gi, gq), "nx = 0": (_desc(art, nx=0), gm, gi, gq), "2^32 pixels": (_desc(art, nx=1 << 16, ny=1 << 16), gm, gi, gq),
        "alpha_min = 0": (_desc(art, alpha_min=0.0), gm, gi, gq), "depth_tol nan": (_desc(art, depth_tol=nan), gm, gi, gq),
        "normal_min > 1": (_desc(art, normal_min=2.0), gm, gi, gq), "max_history inf": (_desc(art, max_history=inf), gm, gi, gq),
        "null color": (_desc(art, color=None), gm, gi, gq), "null depth": (_desc(art, depth=None), gm, gi, gq),
        "null alpha": (_desc(art, alpha=None), gm, gi, gq), "null out": (_desc(art, out=None), gm, gi, gq),
        "null out_len": (_desc(art, out_len=None), gm, gi, gq), "history without len": (_desc(art, history_len=None), gm, gi, gq),
        "len without history": (_desc(art, history=False, history_len=FAKE * 12), gm, _instances(art, history=False), gq),
        "singular prev": (_desc(art, prev=singular), gm, gi, gq), "out is color": (_desc(art, out=FAKE), gm, gi, gq),
        "motion overlaps out": (_desc(art, motion=FAKE * 4 + 128), gm, gi, gq),
        # rt_reproject_moving's
        "null m": (_desc(art), None, gi, gq), "null prim": (_desc(art, prim=None), gm, gi, gq), "null prev_prim": (_desc(art, prev_prim=None), gm, gi, gq),
        "n_spheres < 0": (_desc(art), _motion(art, n_spheres=-1), gi, gq), "n_media < 0": (_desc(art), _motion(art, n_media=-3), gi, gq),
        "null spheres": (_desc(art), _motion(art, spheres=None), gi, gq), "null prev_spheres": (_desc(art), _motion(art, prev_spheres=None), gi, gq),
        "null media": (_desc(art), _motion(art, media=None), gi, gq),
        "2^28 spheres": (_desc(art), _motion(art, n_spheres=1 << 28), gi, gq), "2^28 media": (_desc(art), _motion(art, n_media=1 << 28), gi, gq),
        "time nan": (_desc(art), _motion(art, time=nan), gi, gq), "prev_time inf": (_desc(art), _motion(art, prev_time=-inf), gi, gq),
        "out overlaps spheres": (_desc(art, out=FAKE * 20 + 32), gm, gi, gq), "motion overlaps media": (_desc(art, motion=FAKE * 22 + 8), gm, gi, gq),
        # rt_reproject_instances'
        "null im": (_desc(art), gm, None, gq), "null inst": (_desc(art), gm, _instances(art, inst=None), gq),
        "history without prev_inst": (_desc(art), gm, _instances(art, prev_inst=None), gq),
        "prev_inst without history": (_desc(art, history=False), gm, _instances(art), gq),
        "n_instances < 0": (_desc(art), gm, _instances(art, n_instances=-1), gq), "2^28 instances": (_desc(art), gm, _instances(art, n_instances=1 << 28), gq),
        "null instances": (_desc(art), gm, _instances(art, instances=None), gq), "null prev_instances": (_desc(art), gm, _instances(art, prev_instances=None), gq),
        "out overlaps instances": (_desc(art, out=FAKE * 30 + 32), gm, gi, gq), "out_len is prev_instances": (_desc(art, out_len=FAKE * 31), gm, gi, gq),
        "motion overlaps inst": (_desc(art, motion=FAKE * 32 + 8), gm, gi, gq), "out overlaps prev_inst": (_desc(art, out=FAKE * 33 + 4), gm, gi, gq),
        # its own
        "null qm": (_desc(art), gm, gi, None),
        "n_quads < 0": (_desc(art), gm, gi, _quads(art, n_quads=-1)), "2^28 quads": (_desc(art), gm, gi, _quads(art, n_quads=1 << 28)),
        "null quads": (_desc(art), gm, gi, _quads(art, quads=None)), "null prev_quads": (_desc(art), gm, gi, _quads(art, prev_quads=None)),
        "out overlaps quads": (_desc(art, out=FAKE * 40 + 80), gm, gi, gq), "out_len is prev_quads": (_desc(art, out_len=FAKE * 41), gm, gi, gq),
        "motion overlaps the last quad": (_desc(art, motion=FAKE * 40 + 10 * 80 - 4), gm, gi, gq),
    }
    texts = {}
    for name, (d, m, im, qm) in cases.items():
        for on_device in (0, 1):
            st = L.rt_reproject_quads(*(None if x is None else C.byref(x) for x in (d, m, im, qm)), on_device, None, 1)
            text = L.rt_last_error_detail().decode()
            assert st == RT_ERR_INVALID and text.startswith("rt_reproject_quads"), (name, on_device, st, text)
        texts[name] = text
    same = [("null prim", "null prev_prim"), ("n_spheres < 0", "n_media < 0"), ("null spheres", "null prev_spheres"), ("2^28 spheres", "2^28 media"),
            ("time nan", "prev_time inf"), ("history without prev_inst", "prev_inst without history"), ("null instances", "null prev_instances"),
            ("null quads", "null prev_quads")]
    for group in same:
        assert len({texts[k] for k in group}) == 1, group
    distinct = [g[0] for g in same] + [k for k in cases if not any(k in g for g in same)]
    assert len({texts[k] for k in distinct}) == len(distinct), texts
    for name, what in (("out overlaps spheres", "spheres"), ("out overlaps instances", "instances"), ("out overlaps prev_inst", "prev_inst"),
                       ("out overlaps quads", "quads"), ("out_len is prev_quads", "prev_quads"), ("motion overlaps the last quad", "quads")):
        assert texts[name].endswith("overlaps " + what), (name, texts[name])
    assert "quad description" in texts["null qm"] and "instance description" in texts["null im"] and "motion description" in texts["null m"]
    assert "negative" in texts["n_quads < 0"] and "2^28" in texts["2^28 quads"] and "prev_quads" in texts["null quads"]
    # what passes: empty tables (null or not), no spheres, no instances, no history, every guide, a buffer just behind a table
    nothing = _motion(art, n_spheres=0, spheres=None, prev_spheres=None, n_media=0, media=None)
    no_inst = _instances(art, n_instances=0, instances=None, prev_instances=None)
    good = [(_desc(art), gm, gi, gq), (_desc(art), nothing, no_inst, gq), (_desc(art), gm, gi, _quads(art, n_quads=0, quads=None, prev_quads=None)),
            (_desc(art), nothing, no_inst, _quads(art, n_quads=0)), (_desc(art, history=False), gm, _instances(art, history=False), gq),
            (_desc(art, normal=FAKE * 14, prev_normal=FAKE * 15, motion=FAKE * 40 + 10 * 80), gm, gi, gq),
            (_desc(art), gm, gi, _quads(art, n_quads=(1 << 28) - 1, quads=FAKE * (1 << 16), prev_quads=FAKE * (1 << 17)))]
    for k, (d, m, im, qm) in enumerate(good):
        if art._initialised_device is None:
            for on_device in (0, 1):
                st = L.rt_reproject_quads(C.byref(d), C.byref(m), C.byref(im), C.byref(qm), on_device, None, 1)
                assert st == RT_ERR_NO_DEVICE, (k, on_device, st, L.rt_last_error_detail().decode())
        else:
            st = L.rt_reproject_quads(C.byref(d), C.byref(m), C.byref(im), C.byref(qm), 1, None, 1)
            assert st == RT_ERR_INVALID and "device memory" in L.rt_last_error_detail().decode(), (k, st)
    assert 37 * 29 * 12 < FAKE and 10 * 80 + 37 * 29 * 8 < FAKE and ((1 << 28) - 1) * 80 < FAKE * (1 << 16)


def test_binding_rejects_malformed_quad_arguments_before_any_device_work(art):
    c, z, ids = np.zeros((6, 8, 3), np.float32), np.zeros((6, 8), np.float32), np.zeros((6, 8), np.int32)
    cam = sg.make_camera(*CAMERAS[1], 0.0, 0.0)
    hist = dict(history=c, history_len=z, prev_depth=z, prev_alpha=z)
    qd, ins = np.zeros(3, art.QUAD_DTYPE), np.zeros(3, art.INSTANCE_DTYPE)
    pp = dict(prim=ids, prev_prim=ids)
    bad = [
        lambda: art.reproject(c, z, z, cam, cam, **pp, prev_quads=qd, inst=ids, prev_inst=ids, **hist),                       # no quads
        lambda: art.reproject(c, z, z, cam, cam, **pp, quads=qd, inst=ids, prev_inst=ids, **hist),                            # no prev_quads
        lambda: art.reproject(c, z, z, cam, cam, **pp, quads=qd, prev_quads=qd, prev_inst=ids, **hist),                       # no inst
        lambda: art.reproject(c, z, z, cam, cam, **pp, quads=qd, prev_quads=qd, inst=ids, **hist),                            # no prev_inst
        lambda: art.reproject(c, z, z, cam, cam, **pp, quads=qd, prev_quads=qd, inst=ids, prev_inst=ids),                     # ... without history
        lambda: art.reproject(c, z, z, cam, cam, quads=qd, prev_quads=qd, inst=ids, prev_inst=ids, **hist),                   # no ids
        lambda: art.reproject(c, z, z, cam, cam, **pp, quads=qd, prev_quads=qd[:2], inst=ids, prev_inst=ids, **hist),
        lambda: art.reproject(c, z, z, cam, cam, **pp, quads=qd, prev_quads=ins, inst=ids, prev_inst=ids, **hist),            # the wrong dtype
        lambda: art.reproject(c, z, z, cam, cam, **pp, quads=np.zeros((3, 20), np.float32), prev_quads=qd, inst=ids, prev_inst=ids, **hist),
        lambda: art.reproject(c, z, z, cam, cam, **pp, quads=qd, prev_quads=qd, inst=z, prev_inst=ids, **hist),               # a float plane
        lambda: art.reproject(c, z, z, cam, cam, **pp, quads=qd, prev_quads=qd, inst=ids, prev_inst=ids, prev_instances=ins, **hist),
        lambda: art.reproject(c, z, z, cam, cam, **pp, quads=qd, prev_quads=qd, inst=ids, prev_inst=ids, instances=ins, **hist),
        lambda: art.reproject(c, z, z, cam, cam, **pp, quads=qd, prev_quads=qd, inst=ids, prev_inst=ids, time=float("nan"), **hist),
        lambda: art.TemporalAccumulator(None, art.RtFrameDesc(), follow_quads=True),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")


def test_accumulator_takes_a_quad_update_only_with_the_flag(art):
    """push()'s argument checks come before anything touches the scene: without follow_quads every quad argument is a ValueError,
    as the sphere and instance arguments are without theirs; the three flags are independent."""
    frame = art.RtFrameDesc()
    frame.nx, frame.ny, frame.ns, frame.tile_rows, frame.tile_stride = 8, 6, 2, 6, 1
    cam = sg.make_camera(*CAMERAS[1], 0.0, 0.0)
    acc = art.TemporalAccumulator(None, frame)
    assert (acc.follow_spheres, acc.follow_instances, acc.follow_quads) == (False, False, False)
    for kw in (dict(quads=np.zeros(1, art.QUAD_DTYPE)), dict(quad_indices=np.zeros(1, np.int32)), dict(quad_first=1)):
        with pytest.raises(ValueError, match="follow_quads=True"):
            acc.push(cam, **kw)
    acc = art.TemporalAccumulator(None, frame, follow_instances=True, follow_spheres=True)
    with pytest.raises(ValueError, match="follow_quads=True"):
        acc.push(cam, quads=np.zeros(1, art.QUAD_DTYPE))
    acc = art.TemporalAccumulator(None, frame, follow_quads=True)
    assert (acc.follow_spheres, acc.follow_instances, acc.follow_quads) == (False, False, True)
    with pytest.raises(ValueError, match="follow_instances=True"):
        acc.push(cam, instances=np.zeros(1, art.INSTANCE_DTYPE))
    with pytest.raises(ValueError, match="follow_spheres=True"):
        acc.push(cam, spheres=np.zeros(1, art.SPHERE_DTYPE))


# ------------------------------------------------------------------------------------------------- the restatement itself
def test_no_quad_or_no_differing_record_is_the_instance_restatement_bit_for_bit():
    """n_quads = 0 (no table, empty tables) and tables in which no record differs in Q, u or v -- record 5 still differs in n, w, D,
    mat and the pads --: ix.reproject's bits on the painted planes for every camera, normals on and off, with the moving sphere
    and instance tables in place."""
    s = qx.synthetic_quads(37, 29, 7)
    t = qx.without_quads(s["tables"])
    cur, same = qx.unmoved_quad_tables()
    assert not qx.quad_records_differ(cur, same).any() and cur[5].tobytes() != same[5].tobytes()
    empty = np.zeros(0, qx.QUAD_DTYPE)
    for normals in (False, True):
        kw = qx.select(s["buffers"], normals)
        for name, prev in s["cams"].items():
            want = ix.reproject(cur=s["cur"], prev=prev, **kw, **t)
            for what, tables in (("none", {}), ("empty", dict(quads=empty, prev_quads=empty)), ("unmoved", dict(quads=cur, prev_quads=same))):
                details = {}
                got = qx.reproject(cur=s["cur"], prev=prev, details=details, **kw, **t, **tables)
                assert not details["followed_quad"].any() and details["followed"].any() and details["followed_sphere"].any()
                assert details["on_quad"].any() == (what == "unmoved")
                for g, w, part in zip(got, want, ("out", "out_len", "motion")):
                    assert g.dtype == np.float32 and _same(g, w), (name, what, part, normals)


def test_synthetic_inputs_reach_every_branch():
    """The GPU test's inputs: each rule of the quad tail decides some pixel, and the other two tails still do.  Every count below
    is asserted > 0."""
    s = qx.synthetic_quads(37, 29, 7)
    b, t = s["buffers"], s["tables"]
    n, nq = ix.N_INSTANCES, qx.N_QUADS
    for frame in (b["prim"], b["prev_prim"]):
        assert set(np.unique(frame)) == set(qx.id_palette().tolist())
    for frame in (b["inst"], b["prev_inst"]):
        assert set(np.unique(frame)) == set(ix.inst_palette().tolist())
    surface = b["alpha"] >= 0.5
    inst, prim = b["inst"].astype(np.int64), b["prim"].astype(np.int64)
    kind, index = np.where(prim >= 0, prim >> 28, -1), prim & 0x0FFFFFFF
    details = {}
    near = qx.reproject(cur=s["cur"], prev=s["cams"]["near"], details=details, **b, **t)
    g, fq, i, f, fs = details["quad"], details["followed_quad"], details["instance"], details["followed"], details["followed_sphere"]
    is_quad = kind == qx.QUAD
    imoved = ix.records_differ(t["instances"], t["prev_instances"])
    qmoved = qx.quad_records_differ(t["quads"], t["prev_quads"])
    assert qmoved.tolist() == [True, False, True, True, True, False, True, True, True, True]
    under_moved = (inst >= 0) & (inst < n) & imoved[np.clip(inst, 0, n - 1)]
    under_unmoved = (inst >= 0) & (inst < n) & ~imoved[np.clip(inst, 0, n - 1)]
    counts = {
        "a quad in range with inst -1": (surface & (g >= 0) & (inst == -1)).sum(),
        "a quad in range with a negative inst that is not -1": (surface & (g >= 0) & (inst < -1)).sum(),
        "a moved quad under an unmoved instance": (fq & under_unmoved & ~f).sum(),
        "a moved quad under a moved instance": (fq & under_moved & f).sum(),
        "an unmoved quad under a moved instance: 1c' alone": (surface & (g >= 0) & ~fq & f).sum(),
        "an unmoved quad under an unmoved instance or none: static": (surface & (g >= 0) & ~fq & ~f).sum(),
        "a quad in range with inst >= n_instances: not the quad path": (surface & is_quad & (index < nq) & (inst >= n) & (g == -1)).sum(),
        "a quad index >= n_quads": (surface & is_quad & (index >= nq) & (g == -1)).sum(),
        "a quad index >= n_quads under a moved instance: the instance path": (surface & is_quad & (index >= nq) & f).sum(),
        "a negative prim": (surface & (prim < 0) & (g == -1)).sum(),
        "a sphere followed as one": (fs & (kind == ix.SPHERE)).sum(), "a medium": (surface & (kind == ix.MEDIUM) & (g == -1)).sum(),
        "a medium followed through its boundary": ((f | fs) & (kind == ix.MEDIUM)).sum(),
        "an instance pixel whose prim is a sphere": (f & (kind == ix.SPHERE)).sum(),
        "a box id: not a quad": (surface & (kind == ix.BOX) & (g == -1)).sum(),
        "sky on a moved quad is not followed": (~surface & is_quad & (index < nq) & qmoved[np.clip(index, 0, nq - 1)] & ~fq).sum(),
        "followed and found a history": (fq & (near[1] > 1)).sum(), "followed and found none": (fq & (near[1] == 1)).sum(),
    }
    for r, why in enumerate(qx.QUAD_RECORDS):
        counts[f"record {r} ({why}) on a surface"] = (surface & (g == r)).sum()
        if qmoved[r]:
            counts[f"record {r} ({why}) followed"] = (fq & (g == r)).sum()
            counts[f"record {r} ({why}) followed under an instance"] = (fq & (g == r) & (i >= 0)).sum()
    print({key: int(v) for key, v in counts.items()})
    for key, v in counts.items():
        assert v > 0, key
    assert not fq[np.isin(g, [1, 5])].any() and not fq[~surface].any() and not (fq & fs).any()
    G, H = t["quads"], t["prev_quads"]
    assert (G["Q"][2] != H["Q"][2]).any() and (G["u"][2] == H["u"][2]).all() and (G["v"][2] == H["v"][2]).all()
    assert (G["u"][3] != H["u"][3]).any() and (G["Q"][3] == H["Q"][3]).all() and (G["v"][3] == H["v"][3]).all()
    assert (G["v"][4] != H["v"][4]).any() and (G["Q"][4] == H["Q"][4]).all() and (G["u"][4] == H["u"][4]).all()
    assert all((G[x][5] != H[x][5]).any() for x in ("n", "w")) and G["D"][5] != H["D"][5] and G["mat"][5] != H["mat"][5] and G["pad1"][5] != H["pad1"][5]
    assert np.isnan(G["Q"][6]).any() and np.isinf(H["u"][7]).any() and not G["w"][8].any()
    # what following changes: pixels no tail of the three follows keep rt_reproject_instances' q (their motion), followed ones get another
    plain = ix.reproject(cur=s["cur"], prev=s["cams"]["near"], **b, **qx.without_quads(t))
    assert _same(near[2][~fq], plain[2][~fq]) and _same(near[1][~fq], plain[1][~fq])
    changed = ((near[2].view(np.uint32) != plain[2].view(np.uint32)) & ~(np.isnan(near[2]) & np.isnan(plain[2]))).any(axis=-1)
    assert changed[fq].mean() > 0.9
    for dead in (6, 7):                                                                  # a non-finite carry ends with no history
        assert (near[1][fq & (g == dead)] == 1).all(), dead
    # a zero w: alpha = beta = 0, so P' is the previous record's Q taken out of object space -- finite, wrong and harmless
    zero = fq & (g == 8) & (i < 0)
    assert zero.any()
    B = np.zeros((1, 3), np.float32) + np.float32(7.5)
    assert np.array_equal(qx.carry_point(B, G[8:9], H[8:9]), H["Q"][8:9])
    behind = qx.reproject(cur=s["cur"], prev=s["cams"]["behind"], **b, **t)
    assert (behind[1][surface] == 1).all()
    first = qx.reproject(cur=s["cur"], prev=s["cams"]["near"], **qx.select(b, True, history=False), **t)
    assert _same(first[0], b["color"]) and (first[1] == 1).all() and _same(first[2], near[2])
    # the normal test decides taps of followed pixels (`near` had the normals on: b holds them)
    off = qx.reproject(cur=s["cur"], prev=s["cams"]["near"], **qx.select(b, False), **t)
    assert (off[1][fq] != near[1][fq]).any()


# ------------------------------------------------------------------------------------- the carry against float64
def _moved_face(art):
    """The +x face (face 1 of make_box) of a box that went from [-0.4, 0.4] x [0, 1.1] x [-0.3, 0.3] to [-0.1, 0.9] x [0.2, 0.8] x
    [-0.5, 0.4] -- another position and another size on every axis -- under an instance that was translate(rotate_y(., 15), a) in the
    previous frame and is translate(rotate_y(., -18), b) in the current one; a grid of planar coordinates on it, the edges and a
    little beyond included."""
    a, b = np.array([1.3, 0.0, -2.1], np.float32), np.array([-0.7, 0.25, 1.6], np.float32)
    before, now = ix.record(15.0, a), ix.record(-18.0, b)
    Hq = art.box_records((-0.4, 0.0, -0.3), (0.4, 1.1, 0.3), 0)[1:2]
    G = art.box_records((-0.1, 0.2, -0.5), (0.9, 0.8, 0.4), 0)[1:2]
    assert abs(G["n"][0, 0]) == 1 and G["Q"][0, 0] == np.float32(0.9) and Hq["Q"][0, 0] == np.float32(0.4)
    al, be = np.meshgrid(np.linspace(-0.05, 1.05, 23), np.linspace(-0.05, 1.05, 17), indexing="ij")
    return G, Hq, now, before, al[..., None], be[..., None]


def _rot64(v, rec, inverse=False):
    """rotate_y in float64 with the record's own float sin_t / cos_t: object -> world x' = c x + s z, z' = c z - s x; world ->
    object with inverse=True."""
    c, s = float(rec["cos_t"]), float(rec["sin_t"]) * (-1.0 if inverse else 1.0)
    return np.stack([c * v[..., 0] + s * v[..., 2], v[..., 1], c * v[..., 2] - s * v[..., 0]], axis=-1)


def _f64(rec, name):
    return rec[name][0].astype(np.float64)


def test_carry_of_a_moved_box_face_against_the_affine_map_in_float64(art):
    """A point P of the face as the current frame shows it (object point Q + al u + be v, out by the current instance record,
    rounded to float): the restatement's carried point against the same map -- into object space by the current instance record,
    (alpha, beta) by the current quad record, Q' + alpha u' + beta v' by the previous one, out by the previous instance record --
    evaluated in float64 from the same float records and the same float P.

    The bound.  For an expression of + - * evaluated in binary32 the computed value differs from the exact one by at most
    gamma_k = k u / (1 - k u) times the same expression with every operand and every intermediate replaced by its absolute value,
    u = 2^-24, k the largest number of rounded operations on a path from an input to the result.  On the path of one component of
    P': A = P - offset (1); B = c A.x -+ s A.z (a product and a sum, 2); h = B - Q (1); a component of cross(h, v) (a product and a
    difference, 2); alpha = (w0 x0 + w1 x1) + w2 x2 (a product and two sums, 3); (Q' + alpha u') + beta v' (a product and two sums,
    3); C = c' B' +- s' B' (2); P' = C + offset' (1): k = 15, and 16 u covers gamma_15.  The magnitude is that absolute-value
    expression, evaluated below in float64 (`mag`); float64's own rounding is 2^-29 of the bound."""
    G, Hq, now, before, al, be = _moved_face(art)
    obj = _f64(G, "Q") + al * _f64(G, "u") + be * _f64(G, "v")
    P = (_rot64(obj, now) + now["offset"].astype(np.float64)).astype(np.float32)
    got = qx.to_world(qx.carry_point(qx.to_object(P, now), G, Hq), before).astype(np.float64)
    # the same map in float64
    B = _rot64(P.astype(np.float64) - now["offset"].astype(np.float64), now, inverse=True)
    h = B - _f64(G, "Q")
    alpha, beta = np.cross(h, _f64(G, "v")) @ _f64(G, "w"), np.cross(_f64(G, "u"), h) @ _f64(G, "w")
    want = _rot64(_f64(Hq, "Q") + alpha[..., None] * _f64(Hq, "u") + beta[..., None] * _f64(Hq, "v"), before) + before["offset"].astype(np.float64)
    # ... and with absolute values throughout
    rot_abs = lambda v, rec: np.stack([abs(float(rec["cos_t"])) * v[..., 0] + abs(float(rec["sin_t"])) * v[..., 2], v[..., 1],   # noqa: E731
                                       abs(float(rec["cos_t"])) * v[..., 2] + abs(float(rec["sin_t"])) * v[..., 0]], axis=-1)
    cross_abs = lambda x, y: np.stack([x[..., 1] * y[2] + x[..., 2] * y[1], x[..., 2] * y[0] + x[..., 0] * y[2], x[..., 0] * y[1] + x[..., 1] * y[0]], axis=-1)   # noqa: E731
    habs = rot_abs(np.abs(P).astype(np.float64) + np.abs(now["offset"]).astype(np.float64), now) + np.abs(_f64(G, "Q"))
    aabs = cross_abs(habs, np.abs(_f64(G, "v"))) @ np.abs(_f64(G, "w"))
    babs = cross_abs(habs, np.abs(_f64(G, "u"))) @ np.abs(_f64(G, "w"))
    mag = rot_abs(np.abs(_f64(Hq, "Q")) + aabs[..., None] * np.abs(_f64(Hq, "u")) + babs[..., None] * np.abs(_f64(Hq, "v")), before) \
        + np.abs(before["offset"]).astype(np.float64)
    bound = 16 * U * mag
    err = np.abs(got - want)
    print(f"largest |carried - float64 affine map| / bound {np.max(err / bound):.3f}, largest error {err.max():.3e}, smallest bound {bound.min():.3e}")
    assert (err <= bound).all()
    # the map is the right one: it lands on the face the previous frame showed at the same planar coordinates, up to the float
    # rounding of P, which the map amplifies by no more than the ratio of the sizes
    shown = _rot64(_f64(Hq, "Q") + al * _f64(Hq, "u") + be * _f64(Hq, "v"), before) + before["offset"].astype(np.float64)
    assert np.abs(want - shown).max() < 1e-5
    assert np.abs(want - P).max() > 1.0                                    # whole units, not a rounding matter
    # without an instance it is the plain affine map of the plane, and the instance rule alone would have missed by the resize
    plain = qx.carry_point(obj.astype(np.float32), G, Hq).astype(np.float64)
    assert np.abs(plain - (_f64(Hq, "Q") + al * _f64(Hq, "u") + be * _f64(Hq, "v"))).max() < 1e-5
    assert np.abs(ix.carry_point(P, now, before).astype(np.float64) - shown).max() > 0.3


def test_carried_normal_of_a_moved_box_face_is_the_previous_records_normal(art):
    """The world normal the current frame stored for the face, on either side and with a sample-averaged length below one, against
    s G'.n through the previous rotation in float64, s = dot(Nb, G.n) from the same floats.  The bound by the rule above: Nb = c N.x
    -+ s N.z (2), dot(Nb, G.n) (a product and two sums, 3), s G'.n (1), the previous rotation (2): k = 8, so 8 u / (1 - 8 u) <= 9 u
    times the absolute-value expression.  And it is the right vector: +- length * G'.n through the previous rotation."""
    G, Hq, now, before, _, _ = _moved_face(art)
    for side, length in ((1.0, 1.0), (-1.0, 1.0), (1.0, 0.8125), (-1.0, 0.4375)):
        N = (side * length * _rot64(_f64(G, "n"), now)).astype(np.float32)[None, :]
        got = qx.rotate_out(qx.carry_normal(qx.rotate_in(N, now), G, Hq), before).astype(np.float64)
        Nb = _rot64(N.astype(np.float64), now, inverse=True)
        s64 = Nb @ _f64(G, "n")
        want = _rot64(s64[..., None] * _f64(Hq, "n"), before)
        c, s = abs(float(now["cos_t"])), abs(float(now["sin_t"]))
        Na = np.abs(N).astype(np.float64)
        sabs = np.stack([c * Na[..., 0] + s * Na[..., 2], Na[..., 1], c * Na[..., 2] + s * Na[..., 0]], axis=-1) @ np.abs(_f64(G, "n"))
        hn = sabs[..., None] * np.abs(_f64(Hq, "n"))
        c, s = abs(float(before["cos_t"])), abs(float(before["sin_t"]))
        mag = np.stack([c * hn[..., 0] + s * hn[..., 2], hn[..., 1], c * hn[..., 2] + s * hn[..., 0]], axis=-1)
        assert (np.abs(got - want) <= 9 * U * mag).all(), (side, length, np.abs(got - want).max())
        exact = side * length * _rot64(_f64(Hq, "n"), before)
        assert np.abs(want - exact).max() < 1e-6 and np.abs(s64 - side * length).max() < 1e-6
    # records that did not move leave the normal to rt_reproject_instances' rule; the stored normal is not rotated here at all
    assert np.array_equal(qx.carry_normal(np.array([[0.0, 0.0, 1.0]], np.float32), G, Hq), np.zeros((1, 3), np.float32))   # in the plane: no side
