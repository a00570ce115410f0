"""rt_scene_update_quads on the GPU, test for test as tests/test_update_instances.py: after the call rt_render writes, bit for bit,
what the CPU oracle gives for the changed description D' (tests/refit_quads_expect.py), with and without recalibration, and the
move back restores the first frame; the data the device derives from quad records -- the axis code in pad0, the canonical mark in
bit 30 of first_quad -- equal a fresh scene's after updates that change them; every other frame and query entry equals the same
call on a scene freshly created from D'; the device arrays hold the restatement's boxes by value with every link word untouched;
device-resident records and their device-side check; refusals leave the scene alone; quad, instance and sphere updates on one
scene; rt_multi_update_quads."""
import ctypes as C

import numpy as np
import pytest

import refit_expect as rf
import refit_instances_expect as ri
import refit_quads_expect as rq
import scene_gen as sg

pytestmark = pytest.mark.gpu

SEED = 1984
# cornell: six direct quads (the light among them) and two boxes under instances; cornell_smoke at 32x32: the boxes are boundaries
# of media under instances, the records read through the scalar cache; general_plain/0: a walk array of its own, every way a leaf
# can reach a quad; /2: a medium bounded by a box; /4: one bounded by an instance of a box; limits/12: 13 leaves, one of them the
# scene's only quad; instanced: 128 leaves in two tier slots, quads and boxes under every kind of instance; crowd_big: 8 401
# leaves, no tier data, the whole-slot path of the interior kernel, 15 600 quads replaced at once (1 200 direct ones and the
# faces of 2 400 boxes, half of them under instances)
CASES = {"cornell": ("cornell", 48, 32, 4), "cornell_smoke": ("cornell_smoke", 32, 32, 4), "general": ("general_plain/0", 48, 32, 4),
         "general2": ("general_plain/2", 48, 32, 4), "general4": ("general_plain/4", 48, 32, 4), "limits": ("limits/12", 48, 32, 4),
         "instanced": ("instanced", 48, 32, 4), "crowd_big": ("crowd_big", 48, 32, 4)}
_cache = {}


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} values differ, first at {bad[:3].tolist()}"


def _all_update(scene):
    """`all` of refit_quads_expect for a scene of any size: crowd_big's 15 600 quads take the vectorised form of the same
    update -- every quad displaced, the faces of one box together -- because the restatement's per-quad constructor is a Python
    loop.  Q moves by d, so D = n . Q is made anew as quad::quad makes it; u, v, w and n do not change."""
    if len(scene.quads()) < 1000:
        return rq.make_update(scene, "all")
    quads, boxes = scene.quads(), rq.scene_boxes(scene)
    rng = np.random.default_rng(len(quads))
    size = np.maximum(np.abs(quads["u"]).max(1), np.abs(quads["v"]).max(1)).astype(np.float32)
    step = rng.uniform(-0.15, 0.15, (len(quads), 3)).astype(np.float32)
    for first in boxes:
        step[first:first + 6] = step[first] * np.float32(0.5)
    idx = rng.permutation(len(quads))
    rec = quads[idx]
    rec["Q"] = rec["Q"] + step[idx] * size[idx, None]
    n, Q = rec["n"], rec["Q"]
    rec["D"] = ri.fma32(n[:, 2], Q[:, 2], ri.fma32(n[:, 0], Q[:, 0], n[:, 1] * Q[:, 1]))
    return idx, rec


def _refit(art, scene, idx, rec):
    """D' by the restatement, or for crowd_big by rt_refit_quads (tests/test_update_quads_host.py pins the two equal)."""
    if len(scene.quads()) < 1000:
        nodes, quads, lo, hi = rq.refit(scene, idx, rec)
    else:
        nodes, quads = art.refit_quads(scene.desc, rec, idx)
        leaf = nodes["prim"] >= 0
        lo, hi = nodes["bmin"][leaf], nodes["bmax"][leaf]
    return nodes, quads, lo, hi


def _host(art, key, nx, ny):
    if "/" in key:
        recipe, seed = key.split("/")
        return sg.generate(recipe, int(seed), nx, ny)
    return art.HostScene(key, nx, ny)


def _case(art, orc, name):
    """The scene, its update, D' and the oracle's frames of both; made once."""
    if name not in _cache:
        key, nx, ny, ns = CASES[name]
        scene = _host(art, key, nx, ny)
        idx, rec = _all_update(scene)
        nodes, quads, lo, hi = _refit(art, scene, idx, rec)
        moved = rq.Moved(scene, nodes, quads)
        ref, cnt = orc.OracleScene.from_host(moved, nx, ny).render(ns, seed_base=SEED)
        first, cnt0 = orc.OracleScene.from_host(scene, nx, ny).render(ns, seed_base=SEED)
        assert not np.array_equal(ref, first)                                    # the test sees its own update
        _cache[name] = dict(scene=scene, idx=idx, rec=rec, back=scene.quads()[idx], moved=moved, ref=ref, rays=cnt["rays"], first=first,
                            rays0=cnt0["rays"], frame=scene.frame(nx=nx, ny=ny, ns=ns, seed_base=SEED), nx=nx, ny=ny, ns=ns, lo=lo, hi=hi)
    return _cache[name]


def _boxes(art, ds, which, dtype):
    """rt_debug_scene_boxes: device array `which` of the scene as it stands."""
    n = C.c_size_t(0)
    assert art.rt_lib().rt_debug_scene_boxes(ds._p, which, None, 0, C.byref(n)) == 0
    out = np.zeros(n.value // np.dtype(dtype).itemsize, dtype)
    if n.value:
        assert art.rt_lib().rt_debug_scene_boxes(ds._p, which, out.ctypes.data, out.nbytes, C.byref(n)) == 0
    return out


def _zero_pad0(quads):
    out = quads.copy()
    out["pad0"] = 0
    return out


def _raw_equal(ds, fresh, what):
    """rt_debug_scene_quads, word for word: the records, the axis codes in pad0 and the marks in the box words."""
    (gq, gb), (wq, wb) = ds.debug_quads(), fresh.debug_quads()
    assert np.array_equal(gq["pad0"].view(np.int32), wq["pad0"].view(np.int32)), (what, "axis codes")
    assert gq.tobytes() == wq.tobytes(), (what, "quad records")
    assert np.array_equal(gb, wb), (what, "box words", gb[gb != wb], wb[gb != wb])


@pytest.mark.parametrize("recalibrate", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_render_after_update_equals_the_oracle(gpu, orc, name, recalibrate):
    c = _case(gpu, orc, name)
    ds = gpu.DeviceScene(c["scene"])
    try:
        info = ds.walk_info()
        if name == "general":
            assert info["nodes_walked"] != info["nodes_reference"]               # a walk array of its own
        if name == "crowd_big":
            assert len(c["lo"]) == 8401 and len(c["idx"]) == 15600
        ds.update_quads(c["rec"], c["idx"], recalibrate=recalibrate)
        assert ds.walk_info() == info                                             # the topology is kept
        assert ds.quads().tobytes() == _zero_pad0(c["moved"].quads()).tobytes()
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays"] and st.samples == c["nx"] * c["ny"] * c["ns"], (st.rays, c["rays"], st.samples)
        _same(fb, c["ref"], f"{name} recalibrate={recalibrate}")
        ds.update_quads(c["back"], c["idx"], recalibrate=recalibrate)            # ... and the move back restores the first frame
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays0"]
        _same(fb, c["first"], f"{name} moved back")
    finally:
        ds.close()


@pytest.mark.parametrize("kind", ["one", "tilt", "shear", "grow"])
@pytest.mark.parametrize("name", ["cornell", "general"])
def test_render_after_the_other_updates_equals_the_oracle(gpu, orc, name, kind):
    c = _case(gpu, orc, name)
    idx, rec = rq.make_update(c["scene"], kind)
    moved = rq.moved_scene(c["scene"], idx, rec)
    ref, cnt = orc.OracleScene.from_host(moved, c["nx"], c["ny"]).render(c["ns"], seed_base=SEED)
    assert not np.array_equal(ref, c["first"])
    ds = gpu.DeviceScene(c["scene"])
    try:
        ds.update_quads(rec, idx)
        fb, st = ds.render(c["frame"])
        assert st.rays == cnt["rays"]
        _same(fb, ref, f"{name} {kind}")
        ds.update_quads(c["scene"].quads()[idx], idx)
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays0"]
        _same(fb, c["first"], f"{name} {kind} back")
    finally:
        ds.close()


def _rays(c, n=4096):
    """Rays through the frame from the camera's origin, with times in the shutter."""
    cam = c["scene"].desc.camera
    rng = np.random.default_rng(5)
    s, t = rng.uniform(0, 1, (2, n, 1))
    o = np.tile(np.array(cam.origin, np.float32), (n, 1))
    d = (np.array(cam.lower_left_corner) + s * np.array(cam.horizontal) + t * np.array(cam.vertical) - np.array(cam.origin)).astype(np.float32)
    return o, d, rng.uniform(0, 1, n).astype(np.float32)


def _hits_of(trace, quad_indices):
    """How many rays' closest hit is one of these quads (prim_out names the quad, also for the face of a box)."""
    prim = trace.prim.astype(np.int64)
    return int((((prim >> 28) == sg.QUAD) & (prim >= 0) & np.isin(prim & 0x0FFFFFFF, quad_indices)).sum())


@pytest.mark.parametrize("name", ["cornell", "general"])
def test_marks_follow_the_records(gpu, orc, name):
    """tilt re-marks quads (one code 1..3 -> 0, in `general` also one 0 -> 1..3), shear drops bit 30 of a box and its reverse
    brings it back: after each, the raw device records equal a fresh scene's word for word, and so do the frame and the ray
    queries -- whose rays hit the re-marked quads, by construction: their count on the fresh scene is asserted non-zero."""
    c = _case(gpu, orc, name)
    scene = c["scene"]
    o, d, tm = _rays(c)
    ds = gpu.DeviceScene(scene)
    steps = []
    idx, rec = rq.make_update(scene, "tilt")
    assert len(idx) == (2 if name == "general" else 1)
    steps.append(("tilt", scene, idx, rec))
    tilted = rq.moved_scene(scene, idx, rec)
    sidx, srec = rq.make_update(tilted, "shear")
    steps.append(("shear", tilted, sidx, srec))
    sheared = rq.moved_scene(tilted, sidx, srec)
    steps.append(("unshear", sheared, sidx, tilted.quads()[sidx]))
    try:
        for what, before, idx, rec in steps:
            after = rq.moved_scene(before, idx, rec)
            fresh = gpu.DeviceScene(after)
            try:
                ds.update_quads(rec, idx)
                _raw_equal(ds, fresh, f"{name} {what}")
                wq, wb = rq.device_records(after.quads(), rq.scene_boxes(after))  # ... and the restatement's
                gq, gb = ds.debug_quads()
                assert gq.tobytes() == wq.tobytes() and np.array_equal(gb, wb), (name, what)
                bq, bb = rq.device_records(before.quads(), rq.scene_boxes(before))
                if what == "tilt":
                    assert (bq["pad0"].view(np.int32)[idx] != wq["pad0"].view(np.int32)[idx]).all() and np.array_equal(bb, wb)
                else:
                    assert (bb != wb).sum() == 1                                  # the one box's bit 30
                got, want = ds.trace(o, d, tm, record=True), fresh.trace(o, d, tm, record=True)
                box_first = int(wb[np.flatnonzero(bb != wb)[0]]) & rq.FIRST_MASK if what != "tilt" else None
                watched = idx if what == "tilt" else np.arange(box_first, box_first + 6)
                assert _hits_of(want, watched) > 0, (name, what, "no ray hits the re-marked quads")
                for k in want._fields:
                    _same(getattr(got, k), getattr(want, k), f"{name} {what} trace {k}")
                assert np.array_equal(ds.trace(o, d, tm, any_hit=True), fresh.trace(o, d, tm, any_hit=True))
                fb, st = ds.render(c["frame"])
                fw, sw = fresh.render(c["frame"])
                assert st.rays == sw.rays
                _same(fb, fw, f"{name} {what} frame")
            finally:
                fresh.close()
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["general", "cornell_smoke"])
def test_every_other_entry_equals_a_fresh_scene(gpu, orc, name):
    c = _case(gpu, orc, name)
    ds, fresh = gpu.DeviceScene(c["scene"]), gpu.DeviceScene(c["moved"])
    try:
        ds.update_quads(c["rec"], c["idx"])
        _raw_equal(ds, fresh, name)
        f = c["frame"]
        for what, call in (("aov", lambda s: s.render_aov(f, ids=True)),
                           ("aov_through", lambda s: s.render_aov_through(f, ids=True, through=True, bounces=True))):
            got, want = call(ds), call(fresh)
            assert set(got) == set(want)
            for k in want:
                _same(got[k], want[k], f"{name} {what} {k}")
        got, want = ds.render_adaptive(f, 2, c["ns"], 0.05), fresh.render_adaptive(f, 2, c["ns"], 0.05)
        _same(got[0], want[0], f"{name} adaptive fb")
        _same(got[1], want[1], f"{name} adaptive spp")
        assert (got[2].rays, got[2].samples) == (want[2].rays, want[2].samples)
        got, want = ds.render_variance(f, 2), fresh.render_variance(f, 2)
        _same(got[0], want[0], f"{name} variance fb")
        _same(got[1], want[1], f"{name} variance")
        _same(got[0], c["ref"], f"{name} variance fb against the oracle")
        assert (got[2].rays, got[2].samples) == (want[2].rays, want[2].samples)
        # a progressive frame in two windows
        half = c["ns"] // 2
        outs = []
        for s in (ds, fresh):
            state = gpu.ProgressiveFrame(s, f)
            try:
                state.render(0, half)
                outs.append(state.render(half, c["ns"])[0])
            finally:
                state.close()
        _same(outs[0], outs[1], f"{name} two windows")
        o, d, tm = _rays(c)
        got, want = ds.trace(o, d, tm, record=True), fresh.trace(o, d, tm, record=True)
        assert (want.prim >= 0).sum() > len(o) // 4
        assert _hits_of(want, c["idx"]) > 0                                       # some ray hits an updated quad
        for k in want._fields:
            _same(getattr(got, k), getattr(want, k), f"{name} trace {k}")
        assert np.array_equal(ds.trace(o, d, tm, any_hit=True), fresh.trace(o, d, tm, any_hit=True))
        got, want = ds.radiance(o[:512], d[:512], tm[:512], ns=2, count_rays=True), fresh.radiance(o[:512], d[:512], tm[:512], ns=2, count_rays=True)
        _same(got.rgb, want.rgb, f"{name} radiance rgb")
        _same(got.rays, want.rays, f"{name} radiance rays")
    finally:
        ds.close()
        fresh.close()


# per case: whether the scene has tier data (None: a generated scene says so itself).  instanced: 128 leaves in two tier slots,
# so that the root meets whole slots; crowd_big: head, whole-slot and tail paths of the interior kernel, no tier data.  Between them
# the cases update a leaf of every way a solid depends on a quad -- general: a free quad, a box face, an instance of a quad, an
# instance of a box, a medium bounded by a box; general4 (40 leaves): a medium bounded by an instance of a box
ARRAY_CASES = {"general": None, "general4": None, "limits": None, "cornell": True, "instanced": True, "crowd_big": False}


@pytest.mark.parametrize("name", list(ARRAY_CASES))
def test_device_arrays_hold_the_restatement(gpu, orc, name):
    c = _case(gpu, orc, name)
    scene = c["scene"]
    has_tier = scene.has_tier_data if ARRAY_CASES[name] is None else ARRAY_CASES[name]
    ds, fresh = gpu.DeviceScene(scene), gpu.DeviceScene(c["moved"])
    try:
        before = {w: _boxes(gpu, ds, w, dt) for w, dt in ((0, gpu.NODE_DTYPE), (1, gpu.NODE_DTYPE), (2, np.float32), (3, np.float32))}
        info = ds.walk_info()
        ds.update_quads(c["rec"], c["idx"])
        lo, hi = c["lo"], c["hi"]
        want_ref = c["moved"].nodes()
        want_walk = rq.refit_array(rq.decode_device(before[1]), lo, hi)
        for which, want in ((0, want_ref), (1, want_walk)):
            got = _boxes(gpu, ds, which, gpu.NODE_DTYPE)
            assert np.array_equal(got["skip"], before[which]["skip"]) and np.array_equal(got["prim"], before[which]["prim"]), which
            rq.same_values(got["bmin"], want["bmin"], f"{name} array {which} bmin")
            rq.same_values(got["bmax"], want["bmax"], f"{name} array {which} bmax")
        m = len(lo)
        if name == "crowd_big":
            assert m == 8401 > 128
        tier = [_boxes(gpu, ds, w, np.float32).reshape(-1, 4) for w in (2, 3)]
        assert (len(tier[0]) > 0) == has_tier
        if has_tier:
            for got, want, was in ((tier[0], lo, before[2]), (tier[1], hi, before[3])):
                assert len(got) == (m + 63) // 64 * 64
                rq.same_values(got[:m, :3], want, f"{name} tier leaves")
                assert (got[m:, :3].view(np.uint32) == 0).all()                   # padding leaves stay zero
                assert np.array_equal(got[:, 3].view(np.uint32), was.reshape(-1, 4)[:, 3].view(np.uint32))   # .w untouched
            rq.same_values(_boxes(gpu, ds, 4, np.float32).reshape(-1, 8), rq.slot_ranges(lo, hi), f"{name} slot ranges")
        rq.same_values(_boxes(gpu, ds, 5, np.float32), rq.bound(lo, hi), f"{name} bound")
        rq.same_values(_boxes(gpu, ds, 5, np.float32), _boxes(gpu, fresh, 5, np.float32), f"{name} bound against a fresh scene")
        assert ds.walk_info() == info
        _raw_equal(ds, fresh, name)
    finally:
        ds.close()
        fresh.close()


def _tensor(rec, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.float32).reshape(-1, 20).copy()).to(dev)


def test_device_resident_records(gpu, orc):
    """A torch tensor of records, read in place on a stream other than the current one -- which must wait for the copy that fills
    the tensor -- gives the frame of the numpy update."""
    import torch
    c = _case(gpu, orc, "general")
    ds = gpu.DeviceScene(c["scene"])
    try:
        dev = torch.device("cuda", ds.device)
        t = _tensor(c["rec"], dev)
        ds.update_quads(t, c["idx"], stream=torch.cuda.Stream(dev))
        assert ds.quads().tobytes() == _zero_pad0(c["moved"].quads()).tobytes()
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays"]
        _same(fb, c["ref"], "tensor update on a side stream")
        # a contiguous range without an index list, as int32 words, on the current stream
        first = int(c["idx"].min())
        ds.update_quads(_tensor(c["scene"].quads()[first:first + 2], dev).view(torch.int32), first=first)
        assert ds.quads()[first:first + 2].tobytes() == _zero_pad0(c["scene"].quads()[first:first + 2]).tobytes()
        wide = torch.zeros((len(c["idx"]), 40), dtype=torch.float32, device=dev)
        for bad, match in ((t[:, :8], "expected"), (t.double(), "expected"), (t.t(), "expected"), (wide[:, :20], "contiguous"), (t.cpu(), "tensor on"),
                           ([1.0], "expected")):
            with pytest.raises(ValueError, match=match):
                ds.update_quads(bad, c["idx"])
    finally:
        ds.close()


@pytest.mark.parametrize("fault", ["nan_in_u", "mat_out_of_range"])
def test_a_bad_device_record_is_refused_alone(gpu, orc, fault):
    """One planted bad record in a device tensor: the call reports it, the record is neither stored nor stamped, every other
    record is applied, and every box and mark is consistent with what is stored -- the scene equals a fresh scene of "D' without
    that record", frames and raw records alike.  The bad record is a face of a box, so that the box's mark and its leaf's box
    are made from five new faces and one old."""
    import torch
    c = _case(gpu, orc, "general")
    scene = c["scene"]
    first = int(rq.scene_boxes(scene)[rq.census(scene)["direct_boxes"][0]])
    j = int(np.flatnonzero(c["idx"] == first + 2)[0])
    bad = c["rec"].copy()
    if fault == "nan_in_u":
        bad["u"][j, 0] = np.nan
    else:
        bad["mat"][j] = scene.desc.n_materials
    applied = np.arange(len(bad)) != j
    want = rq.moved_scene(scene, c["idx"][applied], c["rec"][applied])
    ref, cnt = orc.OracleScene.from_host(want, c["nx"], c["ny"]).render(c["ns"], seed_base=SEED)
    ds, fresh = gpu.DeviceScene(scene), gpu.DeviceScene(want)
    try:
        dev = torch.device("cuda", ds.device)
        with pytest.raises(ValueError, match="rt_scene_update_quads: a device-resident record"):
            ds.update_quads(_tensor(bad, dev), c["idx"])
        assert ds.quads().tobytes() == _zero_pad0(want.quads()).tobytes()
        _raw_equal(ds, fresh, fault)
        _, _, lo, hi = rq.refit(scene, c["idx"][applied], c["rec"][applied])
        rq.same_values(_boxes(gpu, ds, 5, np.float32), rq.bound(lo, hi), "bound")
        got = _boxes(gpu, ds, 0, gpu.NODE_DTYPE)
        rq.same_values(got["bmin"], want.nodes()["bmin"], "nodes_ref bmin")
        rq.same_values(got["bmax"], want.nodes()["bmax"], "nodes_ref bmax")
        fb, st = ds.render(c["frame"])
        assert st.rays == cnt["rays"]
        _same(fb, ref, "after the refused record")
    finally:
        ds.close()
        fresh.close()


def test_refusals_leave_the_scene_alone(gpu, orc):
    c = _case(gpu, orc, "general")
    scene = c["scene"]
    ds = gpu.DeviceScene(scene)
    try:
        quads = scene.quads()
        raw = ds.debug_quads()
        fb, _ = ds.render(c["frame"])
        _same(fb, c["first"], "before")
        two = c["idx"][[0, 1, 0]]
        for rec, idx, match in ((c["rec"][[0, 1, 0]], two, "rt_scene_update_quads: a quad index appears twice"),
                                (c["rec"][:1], [len(quads)], "rt_scene_update_quads: quad index out of range"),
                                (c["rec"][:1], [-1], "out of range")):
            with pytest.raises(ValueError, match=match):
                ds.update_quads(rec, idx)
        for field, value, match in (("Q", np.inf, "non-finite"), ("D", np.nan, "non-finite"), ("u", np.nan, "non-finite"), ("v", -np.inf, "non-finite"),
                                    ("w", np.nan, "non-finite"), ("n", np.inf, "non-finite"), ("mat", -1, "quad material out of range"),
                                    ("mat", scene.desc.n_materials, "quad material out of range")):
            bad = c["rec"][:1].copy()
            bad[field] = value
            with pytest.raises(ValueError, match=match):
                ds.update_quads(bad, c["idx"][:1], recalibrate=True)
        L = gpu.rt_lib()
        assert L.rt_scene_update_quads(ds._p, None, 0, 0, None) == 1 and "null update" in L.rt_last_error_detail().decode()
        assert L.rt_scene_update_quads(None, None, 0, 0, None) == 1 and "null scene" in L.rt_last_error_detail().decode()
        u = gpu.RtQuadUpdate()
        u.count = 1
        assert L.rt_scene_update_quads(ds._p, C.byref(u), 0, 0, None) == 1 and "null quad records" in L.rt_last_error_detail().decode()
        u.count = -1
        assert L.rt_scene_update_quads(ds._p, C.byref(u), 0, 0, None) == 1 and "count is negative" in L.rt_last_error_detail().decode()
        ds.update_quads(quads[:0])                                                # count == 0: a successful no-op
        assert ds.quads().tobytes() == _zero_pad0(quads).tobytes()
        now = ds.debug_quads()
        assert now[0].tobytes() == raw[0].tobytes() and np.array_equal(now[1], raw[1])
        fb, _ = ds.render(c["frame"])
        _same(fb, c["first"], "after the refusals")
    finally:
        ds.close()


def test_a_pending_render_is_finished_with_the_old_quads(gpu, orc):
    import torch
    c = _case(gpu, orc, "general")
    ds = gpu.DeviceScene(c["scene"])
    try:
        buf = torch.zeros((c["ny"], c["nx"], 3), dtype=torch.float32, device=torch.device("cuda", ds.device))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        ds.render(c["frame"], out=buf.data_ptr(), stream=side.cuda_stream, blocking=False)
        ds.update_quads(c["rec"], c["idx"])
        st = ds.finish()
        side.synchronize()
        assert st.rays == c["rays0"]
        _same(buf.cpu().numpy(), c["first"], "the pending frame")
        fb, _ = ds.render(c["frame"])
        _same(fb, c["ref"], "the frame after it")
    finally:
        ds.close()


@pytest.mark.parametrize("quads_first", [True, False])
def test_quad_instance_and_sphere_updates_on_one_scene(gpu, orc, quads_first):
    """grow (the six faces of a box under instances), then an instance update of those instances, then a sphere update -- and the
    three in the reverse order -- equal a fresh scene of the final description: the instance leaves kernel reads the quads this
    update stored, and the three stamp arrays do not see each other's epochs (the first update of each kind carries epoch 1)."""
    c = _case(gpu, orc, "general")
    scene = c["scene"]
    qidx, qrec = rq.make_update(scene, "grow")
    box = int(np.flatnonzero(rq.scene_boxes(scene) == int(qidx[0]))[0])
    inst = scene.instances()
    iidx = np.flatnonzero(inst["child"] == sg.ref(sg.BOX, box))
    assert len(iidx) > 1                                                          # one box under several instances
    irec = inst[iidx]
    irec["offset"] += np.array([0.2, 0.0, -0.3], np.float32)
    sidx, srec = rf.make_update(scene, "all")
    # the final description: every leaf recomputed by any of the three takes its rule over the final records
    grown = rq.moved_scene(scene, qidx, qrec)
    n2, inst2, _, _ = ri.refit(grown, iidx, irec)
    turned = rq.Moved(grown, n2, grown.quads(), instances=inst2)
    n3, sph3, lo, hi = rf.refit(turned, sidx, srec)
    final = rq.Moved(turned, n3, turned.quads(), instances=inst2, spheres=sph3)
    ref, cnt = orc.OracleScene.from_host(final, c["nx"], c["ny"]).render(c["ns"], seed_base=SEED)
    assert not np.array_equal(ref, c["first"])
    ds, fresh = gpu.DeviceScene(scene), gpu.DeviceScene(final)
    try:
        if quads_first:
            ds.update_quads(qrec, qidx)
            ds.update_instances(irec, iidx)
            ds.update_spheres(srec, sidx)
        else:
            ds.update_spheres(srec, sidx)
            ds.update_instances(irec, iidx)
            ds.update_quads(qrec, qidx)
        assert ds.spheres().tobytes() == final.spheres().tobytes() and ds.instances().tobytes() == final.instances().tobytes()
        assert ds.quads().tobytes() == _zero_pad0(final.quads()).tobytes()
        _raw_equal(ds, fresh, f"quads first {quads_first}")
        got = _boxes(gpu, ds, 0, gpu.NODE_DTYPE)
        rq.same_values(got["bmin"], n3["bmin"], "nodes_ref bmin")
        rq.same_values(got["bmax"], n3["bmax"], "nodes_ref bmax")
        rq.same_values(_boxes(gpu, ds, 5, np.float32), rq.bound(lo, hi), "bound")
        fb, st = ds.render(c["frame"])
        assert st.rays == cnt["rays"]
        _same(fb, ref, f"three updates, quads first {quads_first}")
        # one more quad update with one record: only that quad's stamp is current, every other box stays
        one_idx, one_rec = rq.make_update(final, "one")
        ds.update_quads(one_rec, one_idx)
        n4, _, _, _ = rq.refit(final, one_idx, one_rec)
        got = _boxes(gpu, ds, 0, gpu.NODE_DTYPE)
        rq.same_values(got["bmin"], n4["bmin"], "nodes_ref bmin after one more")
        rq.same_values(got["bmax"], n4["bmax"], "nodes_ref bmax after one more")
    finally:
        ds.close()
        fresh.close()


def test_multi_update_on_one_gpu(gpu, orc):
    """rt_multi_update_quads: the multi frame after the update is the single-device frame of D', and every rank's share of a
    two-rank partition rendered on the updated scene is, bit for bit, that share of D'."""
    c = _case(gpu, orc, "cornell")
    ms = gpu.MultiScene(c["scene"], 1)
    try:
        ms.update_quads(c["rec"], c["idx"])
        fb, st = ms.render(c["frame"], tile_rows=4)
        assert st.rays == c["rays"]
        _same(fb, c["ref"], "multi")
        with pytest.raises(ValueError, match="twice"):
            ms.update_quads(c["rec"][[0, 0]], c["idx"][[0, 0]])
    finally:
        ms.close()
    ds = gpu.DeviceScene(c["scene"])
    try:
        ds.update_quads(c["rec"], c["idx"])
        for rank in range(2):
            f = c["scene"].frame(nx=c["nx"], ny=c["ny"], ns=c["ns"], seed_base=SEED, tile_rows=4, tile_first=rank, tile_stride=2)
            part, _ = ds.render(f)
            _same(part, c["ref"][gpu.local_rows_to_global(f)], f"rank {rank}")
    finally:
        ds.close()
