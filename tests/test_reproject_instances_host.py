"""rt_reproject_instances without a device: the export, the descriptor's layout against the header, the argument checks that run
before any HIP call, the binding's ValueErrors -- and properties of the restatement itself (tests/reproject_instances_expect.py),
so that the GPU parity test (tests/test_reproject_instances.py) cannot agree with a wrong one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reproject_expect as rx
import reproject_instances_expect as ix
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
    assert ("rt_status rt_reproject_instances(const rt_reproject_desc* d, const rt_reproject_motion_desc* m,\n"
            "                                 const rt_reproject_instance_desc* im, int buffers_on_device, void* stream, int blocking);") in header
    assert "rt_reproject_instances" in art.RT_ABI_SYMBOLS
    assert hasattr(art.rt_lib(), "rt_reproject_instances")
    assert art.INSTANCE_DTYPE == ix.INSTANCE_DTYPE and art.INSTANCE_DTYPE.itemsize == 32
    assert (art.RT_INST_ROTATE_Y, art.RT_INST_TRANSLATE, art.RT_PRIM_INSTANCE) == (ix.ROTATE_Y, ix.TRANSLATE, ix.INSTANCE)


def test_instance_desc_layout_matches_header(art, tmp_path):
    """sizeof and every field offset of rt_reproject_instance_desc as a C compiler lays out include/rt_abi.h."""
    fields = [f for f, _ in art.RtReprojectInstanceDesc._fields_]
    assert fields == ["n_instances", "reserved", "instances", "prev_instances", "inst", "prev_inst"]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(rt_reproject_instance_desc));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof(rt_reproject_instance_desc, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(art.REPO_ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(art.RtReprojectInstanceDesc)
    assert got[1:] == [getattr(art.RtReprojectInstanceDesc, f).offset for f in fields]


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


def test_checks_name_what_failed(art):
    """Everything rt_reproject_moving refuses and every refusal of the instance description: RT_ERR_INVALID with a text of its own
    that starts with the entry's name, on both buffers_on_device values; a description that passes every check ends, in a process
    that has initialised no device, at RT_ERR_NO_DEVICE: the checks come before any HIP call."""
    L = art.rt_lib()
    inf, nan = float("inf"), float("nan")
    singular = sg.make_camera(*CAMERAS[0], 0.0, 0.0)
    singular.vertical[:] = singular.horizontal[:]
    gm, gi = _motion(art), _instances(art)
    cases = {
        # rt_reproject's
        "null d": (None, gm, gi), "nx = 0": (_desc(art, nx=0), gm, gi), "2^32 pixels": (_desc(art, nx=1 << 16, ny=1 << 16), gm, gi),
        "alpha_min = 0": (_desc(art, alpha_min=0.0), gm, gi), "depth_tol nan": (_desc(art, depth_tol=nan), gm, gi),
        "normal_min > 1": (_desc(art, normal_min=2.0), gm, gi), "max_history inf": (_desc(art, max_history=inf), gm, gi),
        "null color": (_desc(art, color=None), gm, gi), "null depth": (_desc(art, depth=None), gm, gi), "null alpha": (_desc(art, alpha=None), gm, gi),
        "null out": (_desc(art, out=None), gm, gi), "null out_len": (_desc(art, out_len=None), gm, gi),
        "history without len": (_desc(art, history_len=None), gm, gi),
        "len without history": (_desc(art, history=False, history_len=FAKE * 12), gm, _instances(art, history=False)),
        "singular prev": (_desc(art, prev=singular), gm, gi), "out is color": (_desc(art, out=FAKE), gm, gi),
        "motion overlaps out": (_desc(art, motion=FAKE * 4 + 128), gm, gi),
        # rt_reproject_moving's
        "null m": (_desc(art), None, gi), "null prim": (_desc(art, prim=None), gm, gi), "null prev_prim": (_desc(art, prev_prim=None), gm, gi),
        "n_spheres < 0": (_desc(art), _motion(art, n_spheres=-1), gi), "n_media < 0": (_desc(art), _motion(art, n_media=-3), gi),
        "null spheres": (_desc(art), _motion(art, spheres=None), gi), "null prev_spheres": (_desc(art), _motion(art, prev_spheres=None), gi),
        "null media": (_desc(art), _motion(art, media=None), gi),
        "2^28 spheres": (_desc(art), _motion(art, n_spheres=1 << 28), gi), "2^28 media": (_desc(art), _motion(art, n_media=1 << 28), gi),
        "time nan": (_desc(art), _motion(art, time=nan), gi), "prev_time inf": (_desc(art), _motion(art, prev_time=-inf), gi),
        "out overlaps spheres": (_desc(art, out=FAKE * 20 + 32), gm, gi), "motion overlaps media": (_desc(art, motion=FAKE * 22 + 8), gm, gi),
        # its own
        "null im": (_desc(art), gm, None), "null inst": (_desc(art), gm, _instances(art, inst=None)),
        "history without prev_inst": (_desc(art), gm, _instances(art, prev_inst=None)),
        "prev_inst without history": (_desc(art, history=False), gm, _instances(art)),
        "n_instances < 0": (_desc(art), gm, _instances(art, n_instances=-1)), "2^28 instances": (_desc(art), gm, _instances(art, n_instances=1 << 28)),
        "null instances": (_desc(art), gm, _instances(art, instances=None)), "null prev_instances": (_desc(art), gm, _instances(art, prev_instances=None)),
        "out overlaps instances": (_desc(art, out=FAKE * 30 + 32), gm, gi), "out_len is prev_instances": (_desc(art, out_len=FAKE * 31), gm, gi),
        "motion overlaps inst": (_desc(art, motion=FAKE * 32 + 8), gm, gi), "out overlaps prev_inst": (_desc(art, out=FAKE * 33 + 4), gm, gi),
    }
    texts = {}
    for name, (d, m, im) in cases.items():
        for on_device in (0, 1):
            st = L.rt_reproject_instances(None if d is None else C.byref(d), None if m is None else C.byref(m), None if im is None else C.byref(im),
                                          on_device, None, 1)
            text = L.rt_last_error_detail().decode()
            assert st == RT_ERR_INVALID and text.startswith("rt_reproject_instances"), (name, on_device, st, text)
        texts[name] = text
    same = [("null prim", "null prev_prim"), ("n_spheres < 0", "n_media < 0"), ("null spheres", "null prev_spheres"), ("2^28 spheres", "2^28 media"),
            ("time nan", "prev_time inf"), ("history without prev_inst", "prev_inst without history"), ("null instances", "null prev_instances")]
    for group in same:
        assert len({texts[k] for k in group}) == 1, group
    distinct = [g[0] for g in same] + [k for k in cases if not any(k in g for g in same)]
    assert len({texts[k] for k in distinct}) == len(distinct), texts
    for name, what in (("out overlaps spheres", "spheres"), ("motion overlaps media", "media"), ("out overlaps instances", "instances"),
                       ("out_len is prev_instances", "prev_instances"), ("motion overlaps inst", "inst"), ("out overlaps prev_inst", "prev_inst")):
        assert texts[name].endswith("overlaps " + what), (name, texts[name])
    assert "instance description" in texts["null im"] and "inst" in texts["null inst"] and "prev_inst" in texts["history without prev_inst"]
    assert "negative" in texts["n_instances < 0"] and "2^28" in texts["2^28 instances"] and "prev_instances" in texts["null instances"]
    # what passes: empty tables (null or not), no spheres, no history, every guide, flags of any value are data
    nothing = _motion(art, n_spheres=0, spheres=None, prev_spheres=None, n_media=0, media=None)
    good = [(_desc(art), gm, gi), (_desc(art), nothing, gi), (_desc(art), gm, _instances(art, n_instances=0, instances=None, prev_instances=None)),
            (_desc(art), nothing, _instances(art, n_instances=0)), (_desc(art, history=False), gm, _instances(art, history=False)),
            (_desc(art, normal=FAKE * 14, prev_normal=FAKE * 15, motion=FAKE * 16), gm, gi),
            (_desc(art), gm, _instances(art, n_instances=(1 << 28) - 1, instances=FAKE * 4096, prev_instances=FAKE * 16384, inst=FAKE * 40000,
                                        prev_inst=FAKE * 40001))]
    for k, (d, m, im) in enumerate(good):
        if art._initialised_device is None:
            for on_device in (0, 1):
                st = L.rt_reproject_instances(C.byref(d), C.byref(m), C.byref(im), on_device, None, 1)
                assert st == RT_ERR_NO_DEVICE, (k, on_device, st, L.rt_last_error_detail().decode())
        else:
            st = L.rt_reproject_instances(C.byref(d), C.byref(m), C.byref(im), 1, None, 1)
            assert st == RT_ERR_INVALID and "device memory" in L.rt_last_error_detail().decode(), (k, st)
    assert 37 * 29 * 12 < FAKE and 12 * 32 < FAKE


def test_binding_rejects_malformed_instance_arguments_before_any_device_work(art):
    c, z, ids = np.zeros((6, 8, 3), np.float32), np.zeros((6, 8), np.float32), np.zeros((6, 8), np.int32)
    cam = sg.make_camera(*CAMERAS[1], 0.0, 0.0)
    hist = dict(history=c, history_len=z, prev_depth=z, prev_alpha=z)
    ins, sph = np.zeros(3, art.INSTANCE_DTYPE), np.zeros(3, art.SPHERE_DTYPE)
    pp = dict(prim=ids, prev_prim=ids)
    bad = [
        lambda: art.reproject(c, z, z, cam, cam, **pp, inst=ids, prev_inst=ids, **hist),                                        # planes need instances
        lambda: art.reproject(c, z, z, cam, cam, **pp, prev_instances=ins, **hist),
        lambda: art.reproject(c, z, z, cam, cam, **pp, instances=ins, inst=ids, prev_inst=ids, **hist),                         # no prev_instances
        lambda: art.reproject(c, z, z, cam, cam, **pp, instances=ins, prev_instances=ins, prev_inst=ids, **hist),               # no inst
        lambda: art.reproject(c, z, z, cam, cam, **pp, instances=ins, prev_instances=ins, inst=ids, **hist),                    # no prev_inst
        lambda: art.reproject(c, z, z, cam, cam, **pp, instances=ins, prev_instances=ins, inst=ids, prev_inst=ids),             # ... without history
        lambda: art.reproject(c, z, z, cam, cam, instances=ins, prev_instances=ins, inst=ids, prev_inst=ids, **hist),           # no ids
        lambda: art.reproject(c, z, z, cam, cam, **pp, instances=ins, prev_instances=ins[:2], inst=ids, prev_inst=ids, **hist),
        lambda: art.reproject(c, z, z, cam, cam, **pp, instances=ins, prev_instances=sph, inst=ids, prev_inst=ids, **hist),     # the wrong dtype
        lambda: art.reproject(c, z, z, cam, cam, **pp, instances=np.zeros((3, 8), np.float32), prev_instances=ins, inst=ids, prev_inst=ids, **hist),
        lambda: art.reproject(c, z, z, cam, cam, **pp, instances=ins, prev_instances=ins, inst=z, prev_inst=ids, **hist),       # a float plane
        lambda: art.reproject(c, z, z, cam, cam, **pp, instances=ins, prev_instances=ins, inst=ids[:3], prev_inst=ids, **hist),
        lambda: art.reproject(c, z, z, cam, cam, **pp, instances=ins, prev_instances=ins, inst=ids, prev_inst=ids, prev_spheres=sph, **hist),
        lambda: art.reproject(c, z, z, cam, cam, **pp, instances=ins, prev_instances=ins, inst=ids, prev_inst=ids, time=float("nan"), **hist),
        lambda: art.TemporalAccumulator(None, art.RtFrameDesc(), follow_instances=True),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")


# ------------------------------------------------------------------------------------------------- the restatement itself
def test_no_instance_or_no_differing_record_is_the_sphere_restatement_bit_for_bit():
    """n_instances = 0 on the painted inst planes -- with the inst test of a tap applied to mx's result by hand it cannot differ,
    so the comparison is made where inst is -1 everywhere -- and unmoved tables with inst = -1 everywhere: mx.reproject's bits for
    every camera, normals on and off, with the moving sphere tables in place."""
    s = ix.synthetic_instances(37, 29, 7)
    t = s["tables"]
    none = np.full((29, 37), -1, np.int32)
    b = dict(s["buffers"], inst=none, prev_inst=none)
    spheres = {k: t[k] for k in ("spheres", "prev_spheres", "media", "time", "prev_time")}
    cur, same, _ = ix.unmoved_instance_tables()
    empty = np.zeros(0, ix.INSTANCE_DTYPE)
    for normals in (False, True):
        kw = ix.select(b, normals)
        for name, prev in s["cams"].items():
            want = mx.reproject(cur=s["cur"], prev=prev, **ix.without_inst(kw), **spheres)
            for what, tables in (("none", {}), ("empty", dict(instances=empty, prev_instances=empty)), ("unmoved", dict(instances=cur, prev_instances=same))):
                details = {}
                got = ix.reproject(cur=s["cur"], prev=prev, details=details, **kw, **spheres, **tables)
                assert not details["followed"].any() and details["followed_sphere"].any()
                for g, w, part in zip(got, want, ("out", "out_len", "motion")):
                    assert g.dtype == np.float32 and _same(g, w), (name, what, part, normals)
    # unmoved tables on the painted planes: the media bounded by instances still find their (unmoved) records
    details = {}
    ix.reproject(cur=s["cur"], prev=s["cams"]["near"], details=details, **s["buffers"], **spheres, instances=cur, prev_instances=same)
    assert details["on_instance"].any() and not details["followed"].any()
    # and by mx's own identity the static restatement, with no table at all
    for name, prev in s["cams"].items():
        got = ix.reproject(cur=s["cur"], prev=prev, **b)
        want = rx.reproject(cur=s["cur"], prev=prev, **ix.without_inst(b))
        assert all(_same(g, w) for g, w in zip(got, want)), name


def test_synthetic_inputs_reach_every_branch():
    """The GPU test's inputs: each rule of both tails decides some pixel.  Every count below is asserted > 0."""
    s = ix.synthetic_instances(37, 29, 7)
    b, t = s["buffers"], s["tables"]
    n, media = ix.N_INSTANCES, t["media"]
    for frame in (b["prim"], b["prev_prim"]):
        assert set(np.unique(frame)) == set(ix.id_palette().tolist())
    for frame in (b["inst"], b["prev_inst"]):
        assert set(np.unique(frame)) == set(ix.inst_palette().tolist())
    assert (b["prim"] != b["prev_prim"]).any() and (b["inst"] != b["prev_inst"]).any()
    surface = b["alpha"] >= 0.5
    inst, prim = b["inst"].astype(np.int64), b["prim"].astype(np.int64)
    kind, index = np.where(prim >= 0, prim >> 28, -1), prim & 0x0FFFFFFF
    in_medium = (kind == ix.MEDIUM) & (index < len(media))
    bnd = media["boundary"][np.where(in_medium, index, 0)].astype(np.int64)
    bkind, bindex = np.where(in_medium & (bnd >= 0), bnd >> 28, -1), bnd & 0x0FFFFFFF
    details = {}
    near = ix.reproject(cur=s["cur"], prev=s["cams"]["near"], details=details, **b, **t)
    i, f, k, fs = details["instance"], details["followed"], details["sphere"], details["followed_sphere"]
    counts = {
        "inst in range": (surface & (inst >= 0) & (inst < n)).sum(), "inst -1": (surface & (inst == -1)).sum(),
        "inst >= n_instances": (surface & (inst >= n)).sum(), "inst negative but not -1": (surface & (inst < -1)).sum(),
        "medium bounded by an instance in range": (surface & (inst < 0) & (bkind == ix.INSTANCE) & (bindex < n) & (i == bindex)).sum(),
        "medium bounded by an instance out of range": (surface & (inst < 0) & (bkind == ix.INSTANCE) & (bindex >= n) & (i == -1)).sum(),
        "medium bounded by a sphere, followed as one": (surface & (inst < 0) & (bkind == ix.SPHERE) & fs).sum(),
        "medium bounded by a quad": (surface & (inst < 0) & (bkind == ix.QUAD) & (i == -1) & (k == -1)).sum(),
        "medium with an inst of its own, which wins": (surface & (inst >= 0) & (inst < n) & (bkind == ix.INSTANCE) & (bindex < n) & (bindex != inst) & (i == inst)).sum(),
        "moved sphere id under an instance: the instance path": (surface & (i >= 0) & (kind == ix.SPHERE) & np.isin(index, [0, 9]) & ~fs).sum(),
        "moved sphere id under an inst out of range: the sphere path": (surface & (inst >= n) & (kind == ix.SPHERE) & np.isin(index, [0, 9]) & fs).sum(),
        "sky on an instance is not followed": (~surface & (inst >= 0) & (inst < n) & ~f).sum(),
        "followed and found a history": (f & (near[1] > 1)).sum(), "followed and found none": (f & (near[1] == 1)).sum(),
        "sphere-followed and found a history": (fs & (near[1] > 1)).sum(),
    }
    for r, why in enumerate(ix.INSTANCE_RECORDS):
        counts[f"record {r} ({why}) on a surface"] = (surface & (i == r)).sum()
        if r != 1:
            counts[f"record {r} ({why}) followed"] = (f & (i == r)).sum()
    print({key: int(v) for key, v in counts.items()})
    for key, v in counts.items():
        assert v > 0, key
    assert not f[i == 1].any() and not f[~surface].any() and not (f & fs).any()
    I, J = t["instances"], t["prev_instances"]
    assert I[1] == J[1] and (I["offset"][2] != J["offset"][2]).any() and I["sin_t"][2] == J["sin_t"][2] and I["flags"][2] == J["flags"][2]
    assert (I["offset"][3] == J["offset"][3]).all() and I["sin_t"][3] != J["sin_t"][3]
    for r, (a, p) in ((4, (3, 2)), (5, (1, 3)), (6, (0, 0)), (7, (7, 7))):
        assert (I["flags"][r], J["flags"][r]) == (a, p), r
    for r in (4, 5):
        assert I["sin_t"][r] == J["sin_t"][r] and I["cos_t"][r] == J["cos_t"][r] and (I["offset"][r] == J["offset"][r]).all()
    assert np.isnan(I["sin_t"][8]) and np.isinf(J["offset"][9]).any()
    assert abs(float(I["sin_t"][10]) ** 2 + float(I["cos_t"][10]) ** 2 - 1) > 0.1 and abs(float(J["sin_t"][10]) ** 2 + float(J["cos_t"][10]) ** 2 - 1) > 0.1
    # what following changes: static pixels keep rt_reproject_moving's q (their motion), followed ones get another
    spheres = {key: t[key] for key in ("spheres", "prev_spheres", "media", "time", "prev_time")}
    moving = mx.reproject(cur=s["cur"], prev=s["cams"]["near"], **ix.without_inst(b), **spheres)
    no_sphere = ~(surface & (i >= 0) & (mx.followed_sphere(b["prim"], mx.N_SPHERES, media) >= 0))   # (an instance takes a sphere's carry away)
    plain = ~f & no_sphere
    assert _same(near[2][plain], moving[2][plain])
    changed = ((near[2].view(np.uint32) != moving[2].view(np.uint32)) & ~(np.isnan(near[2]) & np.isnan(moving[2]))).any(axis=-1)
    assert changed[f & (i != 6)].mean() > 0.9
    assert (f & (i == 6) & no_sphere).any() and not changed[f & (i == 6) & no_sphere].any()      # flags 0: moved by the rule, carried by nothing
    for dead in (8, 9):                                                                  # a non-finite carry ends with no history
        assert (near[1][f & (i == dead)] == 1).all(), dead
    behind = ix.reproject(cur=s["cur"], prev=s["cams"]["behind"], **b, **t)
    assert (behind[1][surface] == 1).all()
    first = ix.reproject(cur=s["cur"], prev=s["cams"]["near"], **ix.select(b, True, history=False), **t)
    assert _same(first[0], b["color"]) and (first[1] == 1).all() and _same(first[2], near[2])
    # the normal test decides taps of followed pixels (`near` had the normals on: b holds them)
    off = ix.reproject(cur=s["cur"], prev=s["cams"]["near"], **ix.select(b, False), **t)
    assert (off[1][f] != near[1][f]).any()


def _box_face():
    """A grid of points on the +x face of the box [-0.4, 0.4] x [0, 1.1] x [-0.3, 0.3] in object space, its outward normal, and the
    two records: the previous frame saw translate(rotate_y(box, 15), a), the current one translate(rotate_y(box, -18), b)."""
    a, b = np.array([1.3, 0.0, -2.1], np.float32), np.array([-0.7, 0.25, 1.6], np.float32)
    before, now = ix.record(15.0, a), ix.record(-18.0, b)
    yy, zz = np.meshgrid(np.linspace(0.0, 1.1, 23), np.linspace(-0.3, 0.3, 17), indexing="ij")
    obj = np.stack([np.full(yy.shape, 0.4), yy, zz], axis=-1)
    return obj, np.array([1.0, 0.0, 0.0]), now, before, a, b


def _to_world(v, rec, translate=True):
    """translate(rotate_y(.)) in float64 with the record's own float sin_t / cos_t: x' = c x + s z, z' = c z - s x."""
    c, s = float(rec["cos_t"]), float(rec["sin_t"])
    out = np.stack([c * v[..., 0] + s * v[..., 2], v[..., 1], c * v[..., 2] - s * v[..., 0]], axis=-1)
    return out + rec["offset"].astype(np.float64) if translate else out


def test_carry_of_a_box_face_against_the_rigid_map_in_float64():
    """A point P on the face as the current frame shows it, P = R(-18) p + b rounded to float: the restatement's carried point
    against R(15) R(-18)^-1 (P - b) + a in float64 with the same float sin_t / cos_t values.  The bound 32 * 2^-24 * (|P|inf +
    |a|inf + |b|inf): at most 12 rounded operations lie on any component's path (a subtraction, two products and a sum, two
    products and a sum again, an addition, and the roundings of their operands), each on an intermediate no larger than twice
    that sum, so 12 * 2 * 2^-24 of it, rounded up to 32."""
    obj, n_obj, now, before, a, b = _box_face()
    P = _to_world(obj, now).astype(np.float32)
    got = ix.carry_point(P, now, before).astype(np.float64)
    c, s = float(now["cos_t"]), float(now["sin_t"])
    A = P.astype(np.float64) - b.astype(np.float64)
    B = np.stack([c * A[..., 0] - s * A[..., 2], A[..., 1], s * A[..., 0] + c * A[..., 2]], axis=-1)
    want = _to_world(B, before)
    bound = 32 * 2.0 ** -24 * (np.abs(P).max(axis=-1) + np.abs(a).max() + np.abs(b).max())
    err = np.abs(got - want).max(axis=-1)
    print(f"largest |carried - float64 rigid map| {err.max():.3e}, smallest bound {bound.min():.3e}")
    assert (err <= bound).all()
    # the map is the right one: it lands on the face the previous frame showed, up to the float rounding of P and of sin / cos
    assert np.abs(want - _to_world(obj, before)).max() < 1e-5
    assert np.abs(want - P).max() > 1.0                                    # whole units, not a rounding matter


def test_carried_normal_of_a_box_face_is_the_previous_frames_normal():
    obj, n_obj, now, before, _, _ = _box_face()
    N = _to_world(n_obj, now, translate=False).astype(np.float32)          # (cos_t, 0, -sin_t), exact in float
    assert N[0] == now["cos_t"] and N[2] == -now["sin_t"]
    got = ix.carry_normal(N, now, before).astype(np.float64)
    want = _to_world(n_obj, before, translate=False)
    assert np.abs(got - want).max() <= 4 * 2.0 ** -24, np.abs(got - want).max()
    assert np.abs(N - want).max() > 0.5                                    # uncarried it is another normal: 33 degrees away
    # records that do not rotate leave it alone, bit for bit
    assert np.array_equal(ix.carry_normal(N, ix.record(None, (1, 2, 3)), ix.record(None, (3, 2, 1))), N)
