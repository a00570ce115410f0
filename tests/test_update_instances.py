"""rt_scene_update_instances on the GPU, test for test as tests/test_update_spheres.py: after the call rt_render writes, bit for
bit, what the CPU oracle gives for the changed description D' (tests/refit_instances_expect.py), with and without
recalibration, and the move back restores the first frame; every other frame and query entry equals the same call on a scene
freshly created from D'; the device arrays hold the restatement's boxes by value with every link word untouched;
device-resident records, their stream ordering and their device-side check; refusals leave the scene alone;
rt_multi_update_instances; sphere and instance updates on one scene."""
import ctypes as C

import numpy as np
import pytest

import refit_expect as rf
import refit_instances_expect as ri
import scene_gen as sg

pytestmark = pytest.mark.gpu

SEED = 1984
# instanced: 128 leaves in two tier slots, every instance kind, one child shared by two instances; general_plain/0: a walk array of
# its own; /4 and /5: media bounded by an instanced box and by an instanced moving sphere; cornell_smoke at 32x32: few enough nodes
# for the lockstep scan, the records read through the scalar cache, both instances boundaries of media; small1 .. small25: 1, 2,
# 12, 24 and 25 leaves that hold instances (scene_gen's `limits` recipe has none: ri.small_scene is that recipe with instances);
# crowd_big: 8 401 leaves, no tier data, the whole-slot path of the interior kernel, 1 200 instances updated at once
CASES = {"instanced": ("instanced", 48, 32, 4), "general": ("general_plain/0", 48, 32, 4), "general4": ("general_plain/4", 48, 32, 4),
         "general5": ("general_plain/5", 48, 32, 4), "cornell_smoke": ("cornell_smoke", 32, 32, 4),
         "small1": ("small/1", 48, 32, 4), "small2": ("small/2", 48, 32, 4), "small12": ("small/12", 48, 32, 4),
         "small24": ("small/24", 48, 32, 4), "small25": ("small/25", 48, 32, 4), "crowd_big": ("crowd_big", 48, 32, 2)}
_cache = {}


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} values differ, first at {bad[:3].tolist()}"


def _case(art, orc, name):
    """The scene, its update, D' and the oracle's frames of both; made once."""
    if name not in _cache:
        key, nx, ny, ns = CASES[name]
        if key.startswith("small/"):
            scene = ri.small_scene(int(key.split("/")[1]), 0, nx, ny)
        elif "/" in key:
            recipe, seed = key.split("/")
            scene = sg.generate(recipe, int(seed), nx, ny)
        else:
            scene = art.HostScene(key, nx, ny)
        idx, rec = ri.make_update(scene, "all")
        moved = ri.moved_scene(scene, idx, rec)
        ref, cnt = orc.OracleScene.from_host(moved, nx, ny).render(ns, seed_base=SEED)
        first, cnt0 = orc.OracleScene.from_host(scene, nx, ny).render(ns, seed_base=SEED)
        assert not np.array_equal(ref, first)
        _cache[name] = dict(scene=scene, idx=idx, rec=rec, back=scene.instances()[idx], moved=moved, ref=ref, rays=cnt["rays"], first=first,
                            rays0=cnt0["rays"], frame=scene.frame(nx=nx, ny=ny, ns=ns, seed_base=SEED), nx=nx, ny=ny, ns=ns)
    return _cache[name]


def _boxes(art, ds, which, dtype):
    """rt_debug_scene_boxes: device array `which` of the scene as it stands."""
    n = C.c_size_t(0)
    assert art.rt_lib().rt_debug_scene_boxes(ds._p, which, None, 0, C.byref(n)) == 0
    out = np.zeros(n.value // np.dtype(dtype).itemsize, dtype)
    if n.value:
        assert art.rt_lib().rt_debug_scene_boxes(ds._p, which, out.ctypes.data, out.nbytes, C.byref(n)) == 0
    return out


@pytest.mark.parametrize("recalibrate", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_render_after_update_equals_the_oracle(gpu, orc, name, recalibrate):
    c = _case(gpu, orc, name)
    ds = gpu.DeviceScene(c["scene"])
    try:
        info = ds.walk_info()
        if name == "general":
            assert info["nodes_walked"] != info["nodes_reference"]               # a walk array of its own
        ds.update_instances(c["rec"], c["idx"], recalibrate=recalibrate)
        assert ds.walk_info() == info                                             # the topology is kept
        assert ds.instances().tobytes() == c["moved"].instances().tobytes()
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays"] and st.samples == c["nx"] * c["ny"] * c["ns"], (st.rays, c["rays"], st.samples)
        _same(fb, c["ref"], f"{name} recalibrate={recalibrate}")
        ds.update_instances(c["back"], c["idx"], recalibrate=recalibrate)        # ... and the move back restores the first frame
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays0"]
        _same(fb, c["first"], f"{name} moved back")
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["instanced", "general"])
def test_render_after_a_flags_update_equals_the_oracle(gpu, orc, name):
    """A translate-only instance gains a rotation, a rotated and translated one loses its translation."""
    c = _case(gpu, orc, name)
    idx, rec = ri.make_update(c["scene"], "flags")
    assert len(idx) == 2
    moved = ri.moved_scene(c["scene"], idx, rec)
    ref, cnt = orc.OracleScene.from_host(moved, c["nx"], c["ny"]).render(c["ns"], seed_base=SEED)
    assert not np.array_equal(ref, c["first"])
    ds = gpu.DeviceScene(c["scene"])
    try:
        ds.update_instances(rec, idx)
        fb, st = ds.render(c["frame"])
        assert st.rays == cnt["rays"]
        _same(fb, ref, f"{name} flags")
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


@pytest.mark.parametrize("name", ["instanced", "general"])
def test_every_other_entry_equals_a_fresh_scene(gpu, orc, name):
    c = _case(gpu, orc, name)
    ds, fresh = gpu.DeviceScene(c["scene"]), gpu.DeviceScene(c["moved"])
    try:
        ds.update_instances(c["rec"], c["idx"])
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
        o, d, tm = _rays(c)
        got, want = ds.trace(o, d, tm, record=True), fresh.trace(o, d, tm, record=True)
        assert (want.prim >= 0).sum() > len(o) // 4
        assert np.isin(want.inst[want.inst >= 0], c["idx"]).any()                 # some ray hits an updated instance
        for k in want._fields:
            _same(getattr(got, k), getattr(want, k), f"{name} trace {k}")
        assert np.array_equal(ds.trace(o, d, tm, any_hit=True), fresh.trace(o, d, tm, any_hit=True))
        got, want = ds.radiance(o[:512], d[:512], tm[:512], ns=2, count_rays=True), fresh.radiance(o[:512], d[:512], tm[:512], ns=2, count_rays=True)
        _same(got.rgb, want.rgb, f"{name} radiance rgb")
        _same(got.rays, want.rays, f"{name} radiance rays")
    finally:
        ds.close()
        fresh.close()


# per case: whether the scene has tier data (None: a generated scene says so itself)
ARRAY_CASES = {"instanced": True, "general": None, "general4": None, "cornell_smoke": True, "small25": None, "small1": None, "crowd_big": False}


@pytest.mark.parametrize("name", list(ARRAY_CASES))
def test_device_arrays_hold_the_restatement(gpu, orc, name):
    c = _case(gpu, orc, name)
    scene = c["scene"]
    has_tier = scene.has_tier_data if ARRAY_CASES[name] is None else ARRAY_CASES[name]
    ds, fresh = gpu.DeviceScene(scene), gpu.DeviceScene(c["moved"])
    try:
        before = {w: _boxes(gpu, ds, w, dt) for w, dt in ((0, gpu.NODE_DTYPE), (1, gpu.NODE_DTYPE), (2, np.float32), (3, np.float32))}
        info = ds.walk_info()
        ds.update_instances(c["rec"], c["idx"])
        want_ref, want_inst, lo, hi = ri.refit(scene, c["idx"], c["rec"])
        want_walk, _, _, _ = ri.refit(scene, c["idx"], c["rec"], nodes=ri.decode_device(before[1]))
        for which, want in ((0, want_ref), (1, want_walk)):
            got = _boxes(gpu, ds, which, gpu.NODE_DTYPE)
            assert np.array_equal(got["skip"], before[which]["skip"]) and np.array_equal(got["prim"], before[which]["prim"]), which
            ri.same_values(got["bmin"], want["bmin"], f"{name} array {which} bmin")
            ri.same_values(got["bmax"], want["bmax"], f"{name} array {which} bmax")
        m = len(lo)
        if name == "instanced":
            assert m == 128
        if name == "crowd_big":
            assert m == 8401 and len(c["idx"]) == 1200
        tier = [_boxes(gpu, ds, w, np.float32).reshape(-1, 4) for w in (2, 3)]
        assert (len(tier[0]) > 0) == has_tier
        if has_tier:
            for got, want, was in ((tier[0], lo, before[2]), (tier[1], hi, before[3])):
                assert len(got) == (m + 63) // 64 * 64
                ri.same_values(got[:m, :3], want, f"{name} tier leaves")
                assert (got[m:, :3].view(np.uint32) == 0).all()                   # padding leaves stay zero
                assert np.array_equal(got[:, 3].view(np.uint32), was.reshape(-1, 4)[:, 3].view(np.uint32))   # .w untouched
            ri.same_values(_boxes(gpu, ds, 4, np.float32).reshape(-1, 8), ri.slot_ranges(lo, hi), f"{name} slot ranges")
        ri.same_values(_boxes(gpu, ds, 5, np.float32), ri.bound(lo, hi), f"{name} bound")
        ri.same_values(_boxes(gpu, ds, 5, np.float32), _boxes(gpu, fresh, 5, np.float32), f"{name} bound against a fresh scene")
        assert ds.walk_info() == info
        assert ds.instances().tobytes() == want_inst.tobytes()
        # a far move grows the bound, the move back shrinks it again
        idx, far = ri.make_update(c["moved"], "far")
        ds.update_instances(far, idx)
        _, _, flo, fhi = ri.refit(c["moved"], idx, far)
        ri.same_values(_boxes(gpu, ds, 5, np.float32), ri.bound(flo, fhi), f"{name} bound, far")
        grows = name != "crowd_big"                                               # (its ground reaches 2 000: the far instance stays inside the bound)
        assert (ri.bound(flo, fhi).max() > ri.bound(lo, hi).max()) == grows
        ds.update_instances(c["moved"].instances()[idx], idx)
        _, _, blo, bhi = ri.refit(c["moved"], idx, c["moved"].instances()[idx])
        ri.same_values(_boxes(gpu, ds, 5, np.float32), ri.bound(blo, bhi), f"{name} bound, back")
        assert (ri.bound(blo, bhi).max() < ri.bound(flo, fhi).max()) == grows
        fb, _ = ds.render(c["frame"])
        _same(fb, c["ref"], f"{name} after far and back")
    finally:
        ds.close()
        fresh.close()


def _tensor(rec, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.float32).reshape(-1, 8).copy()).to(dev)


@pytest.mark.parametrize("side_stream", [False, True])
def test_device_resident_records(gpu, orc, side_stream):
    """A torch tensor of records, read in place -- on the current stream, and on another one that must wait for the copy that
    fills the tensor -- gives the frame of the numpy update."""
    import torch
    c = _case(gpu, orc, "general")
    ds = gpu.DeviceScene(c["scene"])
    try:
        dev = torch.device("cuda", ds.device)
        stream = torch.cuda.Stream(dev) if side_stream else None
        t = _tensor(c["rec"], dev)
        ds.update_instances(t, c["idx"], stream=stream)
        assert ds.instances().tobytes() == c["moved"].instances().tobytes()
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays"]
        _same(fb, c["ref"], f"tensor update, side stream {side_stream}")
        # a contiguous range without an index list, as int32 words
        first = int(c["idx"].min())
        ds.update_instances(_tensor(c["scene"].instances()[first:first + 1], dev).view(torch.int32), first=first)
        assert ds.instances()[first].tobytes() == c["scene"].instances()[first].tobytes()
        wide = torch.zeros((len(c["idx"]), 16), dtype=torch.float32, device=dev)
        for bad, match in ((t[:, :7], "expected"), (t.double(), "expected"), (t.t(), "expected"), (wide[:, :8], "contiguous"), (t.cpu(), "tensor on"),
                           ([1.0], "expected")):
            with pytest.raises(ValueError, match=match):
                ds.update_instances(bad, c["idx"])
    finally:
        ds.close()


def test_a_bad_device_record_is_refused_alone(gpu, orc):
    """A NaN offset in a device tensor: the call reports it, the record is not stored, every other record is, and every box is
    consistent with the records actually stored -- the scene equals a fresh scene of the records that were applied.  Bad flags
    and another instance's child are refused the same way."""
    import torch
    c = _case(gpu, orc, "general")
    ds = gpu.DeviceScene(c["scene"])
    try:
        dev = torch.device("cuda", ds.device)
        j = len(c["idx"]) // 3
        bad = c["rec"].copy()
        bad["offset"][j, 1] = np.nan
        applied = np.arange(len(bad)) != j
        with pytest.raises(ValueError, match="device-resident record"):
            ds.update_instances(_tensor(bad, dev), c["idx"])
        want = ri.moved_scene(c["scene"], c["idx"][applied], c["rec"][applied])
        assert ds.instances().tobytes() == want.instances().tobytes()
        _, _, lo, hi = ri.refit(c["scene"], c["idx"][applied], c["rec"][applied])
        ri.same_values(_boxes(gpu, ds, 5, np.float32), ri.bound(lo, hi), "bound")
        got = _boxes(gpu, ds, 0, gpu.NODE_DTYPE)
        ri.same_values(got["bmin"], want.nodes()["bmin"], "nodes_ref bmin")
        ri.same_values(got["bmax"], want.nodes()["bmax"], "nodes_ref bmax")
        ref, cnt = orc.OracleScene.from_host(want, c["nx"], c["ny"]).render(c["ns"], seed_base=SEED)
        fb, st = ds.render(c["frame"])
        assert st.rays == cnt["rays"]
        _same(fb, ref, "after the refused record")
        children = c["scene"].instances()["child"]
        other = children[children != c["rec"]["child"][j]][0]
        for field, value in (("flags", 0), ("flags", 7), ("child", other)):
            bad = c["rec"].copy()
            bad[field][j] = value
            with pytest.raises(ValueError, match="device-resident record"):
                ds.update_instances(_tensor(bad, dev), c["idx"])
            assert ds.instances().tobytes() == want.instances().tobytes()
        fb, _ = ds.render(c["frame"])
        _same(fb, ref, "after the refused flags and child")
    finally:
        ds.close()


def test_refusals_leave_the_scene_alone(gpu, orc):
    c = _case(gpu, orc, "general")
    scene = c["scene"]
    ds = gpu.DeviceScene(scene)
    try:
        inst = scene.instances()
        fb, _ = ds.render(c["frame"])
        _same(fb, c["first"], "before")
        two = c["idx"][[0, 1, 0]]
        for rec, idx, match in ((c["rec"][[0, 1, 0]], two, "rt_scene_update_instances: an instance index appears twice"),
                                (c["rec"][:1], [len(inst)], "rt_scene_update_instances: instance index out of range"),
                                (c["rec"][:1], [-1], "out of range")):
            with pytest.raises(ValueError, match=match):
                ds.update_instances(rec, idx)
        for field, value, match in (("offset", np.inf, "non-finite"), ("sin_t", np.nan, "non-finite"), ("flags", 0, "flags must be 1, 2 or 3"),
                                    ("flags", 4, "flags must be 1, 2 or 3"), ("child", sg.ref(sg.SPHERE, 0) if c["rec"]["child"][0] != sg.ref(sg.SPHERE, 0) else sg.ref(sg.QUAD, 0), "child")):
            bad = c["rec"][:1].copy()
            bad[field] = value
            with pytest.raises(ValueError, match=match):
                ds.update_instances(bad, c["idx"][:1], recalibrate=True)
        L = gpu.rt_lib()
        assert L.rt_scene_update_instances(ds._p, None, 0, 0, None) == 1 and "null update" in L.rt_last_error_detail().decode()
        assert L.rt_scene_update_instances(None, None, 0, 0, None) == 1 and "null scene" in L.rt_last_error_detail().decode()
        u = gpu.RtInstanceUpdate()
        u.count = 1
        assert L.rt_scene_update_instances(ds._p, C.byref(u), 0, 0, None) == 1 and "null instance records" in L.rt_last_error_detail().decode()
        u.count = -1
        assert L.rt_scene_update_instances(ds._p, C.byref(u), 0, 0, None) == 1 and "count is negative" in L.rt_last_error_detail().decode()
        ds.update_instances(inst[:0])                                             # count == 0: a successful no-op
        assert ds.instances().tobytes() == inst.tobytes()
        fb, _ = ds.render(c["frame"])
        _same(fb, c["first"], "after the refusals")
    finally:
        ds.close()


def test_a_pending_render_is_finished_with_the_old_instances(gpu, orc):
    import torch
    c = _case(gpu, orc, "general")
    ds = gpu.DeviceScene(c["scene"])
    try:
        buf = torch.zeros((c["ny"], c["nx"], 3), dtype=torch.float32, device=torch.device("cuda", ds.device))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        ds.render(c["frame"], out=buf.data_ptr(), stream=side.cuda_stream, blocking=False)
        ds.update_instances(c["rec"], c["idx"])
        st = ds.finish()
        side.synchronize()
        assert st.rays == c["rays0"]
        _same(buf.cpu().numpy(), c["first"], "the pending frame")
        fb, _ = ds.render(c["frame"])
        _same(fb, c["ref"], "the frame after it")
    finally:
        ds.close()


def test_multi_update_on_one_gpu(gpu, orc):
    """rt_multi_update_instances: the multi frame after the update is the single-device frame, and so is every rank's share of a
    two-rank partition rendered on the updated scene."""
    c = _case(gpu, orc, "instanced")
    ms = gpu.MultiScene(c["scene"], 1)
    try:
        ms.update_instances(c["rec"], c["idx"])
        fb, st = ms.render(c["frame"], tile_rows=4)
        assert st.rays == c["rays"]
        _same(fb, c["ref"], "multi")
        with pytest.raises(ValueError, match="twice"):
            ms.update_instances(c["rec"][[0, 0]], c["idx"][[0, 0]])
    finally:
        ms.close()
    ds = gpu.DeviceScene(c["scene"])
    try:
        ds.update_instances(c["rec"], c["idx"])
        for rank in range(2):
            f = c["scene"].frame(nx=c["nx"], ny=c["ny"], ns=c["ns"], seed_base=SEED, tile_rows=4, tile_first=rank, tile_stride=2)
            part, _ = ds.render(f)
            _same(part, c["ref"][gpu.local_rows_to_global(f)], f"rank {rank}")
    finally:
        ds.close()


@pytest.mark.parametrize("spheres_first", [True, False])
def test_sphere_and_instance_updates_on_one_scene(gpu, orc, spheres_first):
    """Both updates, in either order, equal a fresh scene of both: the two stamp arrays and their epochs do not interfere (the
    first instance update and the first sphere update carry the same epoch number)."""
    c = _case(gpu, orc, "general")
    scene = c["scene"]
    sidx, srec = rf.make_update(scene, "all")
    with_spheres = rf.moved_scene(scene, sidx, srec)
    nodes, inst, lo, hi = ri.refit(with_spheres, c["idx"], c["rec"])
    both = ri.Moved(with_spheres, nodes, inst, spheres=with_spheres.spheres())
    ref, cnt = orc.OracleScene.from_host(both, c["nx"], c["ny"]).render(c["ns"], seed_base=SEED)
    ds = gpu.DeviceScene(scene)
    try:
        if spheres_first:
            ds.update_spheres(srec, sidx)
            ds.update_instances(c["rec"], c["idx"])
        else:
            ds.update_instances(c["rec"], c["idx"])
            ds.update_spheres(srec, sidx)
        assert ds.spheres().tobytes() == both.spheres().tobytes() and ds.instances().tobytes() == both.instances().tobytes()
        got = _boxes(gpu, ds, 0, gpu.NODE_DTYPE)
        ri.same_values(got["bmin"], nodes["bmin"], "nodes_ref bmin")
        ri.same_values(got["bmax"], nodes["bmax"], "nodes_ref bmax")
        ri.same_values(_boxes(gpu, ds, 5, np.float32), ri.bound(lo, hi), "bound")
        fb, st = ds.render(c["frame"])
        assert st.rays == cnt["rays"]
        _same(fb, ref, f"both updates, spheres first {spheres_first}")
        # an instance update with one record after them: only that instance's stamp is current, the others' boxes stay
        one_idx, one_rec = ri.make_update(both, "one")
        ds.update_instances(one_rec, one_idx)
        n1, _, _, _ = ri.refit(both, one_idx, one_rec)
        got = _boxes(gpu, ds, 0, gpu.NODE_DTYPE)
        ri.same_values(got["bmin"], n1["bmin"], "nodes_ref bmin after one more")
        ri.same_values(got["bmax"], n1["bmax"], "nodes_ref bmax after one more")
    finally:
        ds.close()
