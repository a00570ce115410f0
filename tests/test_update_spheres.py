"""rt_scene_update_spheres on the GPU: after the call rt_render writes, bit for bit, what the CPU oracle gives for the changed
description D' (tests/refit_expect.py), with and without recalibration, and the move back restores the first frame; every other
frame and query entry equals the same call on a scene freshly created from D'; the device arrays hold the restatement's boxes by
value with every link word untouched; device-resident records, their stream ordering and their device-side check; refusals leave
the scene alone; rt_multi_update_spheres."""
import ctypes as C

import numpy as np
import pytest

import refit_expect as rf
import scene_gen as sg

pytestmark = pytest.mark.gpu

SEED = 1984
# spheres_plain/2: 196 leaves, four slots -- head, whole-slot and tail partials all occur; general_plain/0: quads, boxes, instances
# and a sphere-bounded medium, a walk array of its own; media_many: no tier data; limits 0, 1, 2, 4, 5: 1, 2, 12, 24 and 25 leaves
# (scanned in lockstep up to 24 walk nodes, the records read through the scalar cache); the headline scene at 32 spp runs the
# ranked, split schedule, which is what a stale cost prior feeds
CASES = {"spheres": ("spheres_plain/2", 48, 32, 4), "general": ("general_plain/0", 48, 32, 4), "media_many": ("media_many/0", 48, 32, 4),
         "limits1": ("limits/0", 48, 32, 4), "limits2": ("limits/1", 48, 32, 4), "limits12": ("limits/2", 48, 32, 4),
         "limits24": ("limits/4", 48, 32, 4), "limits25": ("limits/5", 48, 32, 4), "headline": ("random_scene", 96, 64, 32)}
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
        if "/" in key:
            recipe, seed = key.split("/")
            scene = sg.generate(recipe, int(seed), nx, ny)
        else:
            scene = art.HostScene(key, nx, ny)
        idx, rec = rf.make_update(scene, "all")
        rec["vel"][::3] = np.array([0.05, 0.3, 0.0], np.float32)      # some of them moving
        moved = rf.moved_scene(scene, idx, rec)
        ref, cnt = orc.OracleScene.from_host(moved, nx, ny).render(ns, seed_base=SEED)
        first, cnt0 = orc.OracleScene.from_host(scene, nx, ny).render(ns, seed_base=SEED)
        assert not np.array_equal(ref, first)
        _cache[name] = dict(scene=scene, idx=idx, rec=rec, back=scene.spheres()[idx], moved=moved, ref=ref, rays=cnt["rays"], first=first,
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
        ds.update_spheres(c["rec"], c["idx"], recalibrate=recalibrate)
        assert ds.walk_info() == info                                             # the topology is kept
        assert ds.spheres().tobytes() == c["moved"].spheres().tobytes()
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays"] and st.samples == c["nx"] * c["ny"] * c["ns"], (st.rays, c["rays"], st.samples)
        _same(fb, c["ref"], f"{name} recalibrate={recalibrate}")
        ds.update_spheres(c["back"], c["idx"], recalibrate=recalibrate)          # ... and the move back restores the first frame
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays0"]
        _same(fb, c["first"], f"{name} moved back")
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


@pytest.mark.parametrize("name", ["spheres", "general"])
def test_every_other_entry_equals_a_fresh_scene(gpu, orc, name):
    c = _case(gpu, orc, name)
    ds, fresh = gpu.DeviceScene(c["scene"]), gpu.DeviceScene(c["moved"])
    try:
        ds.update_spheres(c["rec"], c["idx"])
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
        for k in want._fields:
            _same(getattr(got, k), getattr(want, k), f"{name} trace {k}")
        assert np.array_equal(ds.trace(o, d, tm, any_hit=True), fresh.trace(o, d, tm, any_hit=True))
        got, want = ds.radiance(o[:512], d[:512], tm[:512], ns=2, count_rays=True), fresh.radiance(o[:512], d[:512], tm[:512], ns=2, count_rays=True)
        _same(got.rgb, want.rgb, f"{name} radiance rgb")
        _same(got.rays, want.rays, f"{name} radiance rays")
    finally:
        ds.close()
        fresh.close()


@pytest.mark.parametrize("name", ["spheres", "general", "media_many", "limits25", "limits1"])
def test_device_arrays_hold_the_restatement(gpu, orc, name):
    c = _case(gpu, orc, name)
    scene = c["scene"]
    ds, fresh = gpu.DeviceScene(scene), gpu.DeviceScene(c["moved"])
    try:
        before = {w: _boxes(gpu, ds, w, dt) for w, dt in ((0, gpu.NODE_DTYPE), (1, gpu.NODE_DTYPE), (2, np.float32), (3, np.float32))}
        info = ds.walk_info()
        ds.update_spheres(c["rec"], c["idx"])
        want_ref, want_sph, lo, hi = rf.refit(scene, c["idx"], c["rec"])
        want_walk, _, _, _ = rf.refit(scene, c["idx"], c["rec"], nodes=rf.decode_device(before[1]))
        for which, want in ((0, want_ref), (1, want_walk)):
            got = _boxes(gpu, ds, which, gpu.NODE_DTYPE)
            assert np.array_equal(got["skip"], before[which]["skip"]) and np.array_equal(got["prim"], before[which]["prim"]), which
            rf.same_values(got["bmin"], want["bmin"], f"{name} array {which} bmin")
            rf.same_values(got["bmax"], want["bmax"], f"{name} array {which} bmax")
        m = len(lo)
        tier = [_boxes(gpu, ds, w, np.float32).reshape(-1, 4) for w in (2, 3)]
        assert (len(tier[0]) > 0) == scene.has_tier_data
        if scene.has_tier_data:
            for got, want, was in ((tier[0], lo, before[2]), (tier[1], hi, before[3])):
                assert len(got) == (m + 63) // 64 * 64
                rf.same_values(got[:m, :3], want, f"{name} tier leaves")
                assert (got[m:, :3].view(np.uint32) == 0).all()                   # padding leaves stay zero
                assert np.array_equal(got[:, 3].view(np.uint32), was.reshape(-1, 4)[:, 3].view(np.uint32))   # .w untouched
            rf.same_values(_boxes(gpu, ds, 4, np.float32).reshape(-1, 8), rf.slot_ranges(lo, hi), f"{name} slot ranges")
        rf.same_values(_boxes(gpu, ds, 5, np.float32), rf.bound(lo, hi), f"{name} bound")
        rf.same_values(_boxes(gpu, ds, 5, np.float32), _boxes(gpu, fresh, 5, np.float32), f"{name} bound against a fresh scene")
        assert ds.walk_info() == info
        assert ds.spheres().tobytes() == want_sph.tobytes()
        # a far move grows the bound, the move back shrinks it again
        idx, far = rf.make_update(scene, "far")
        ds.update_spheres(far, idx)
        _, _, flo, fhi = rf.refit(c["moved"], idx, far)
        rf.same_values(_boxes(gpu, ds, 5, np.float32), rf.bound(flo, fhi), f"{name} bound, far")
        assert rf.bound(flo, fhi).max() > rf.bound(lo, hi).max()
        ds.update_spheres(c["moved"].spheres()[idx], idx)
        _, _, blo, bhi = rf.refit(c["moved"], idx, c["moved"].spheres()[idx])
        rf.same_values(_boxes(gpu, ds, 5, np.float32), rf.bound(blo, bhi), f"{name} bound, back")
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
        ds.update_spheres(t, c["idx"], stream=stream)
        assert ds.spheres().tobytes() == c["moved"].spheres().tobytes()
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays"]
        _same(fb, c["ref"], f"tensor update, side stream {side_stream}")
        # a contiguous range without an index list, as int32 words
        first = int(c["idx"].min())
        ds.update_spheres(_tensor(c["scene"].spheres()[first:first + 1], dev).view(torch.int32), first=first)
        assert ds.spheres()[first].tobytes() == c["scene"].spheres()[first].tobytes()
        wide = torch.zeros((len(c["idx"]), 16), dtype=torch.float32, device=dev)
        for bad, match in ((t[:, :7], "expected"), (t.double(), "expected"), (t.t(), "expected"), (wide[:, :8], "contiguous"), (t.cpu(), "tensor on"),
                           ([1.0], "expected")):
            with pytest.raises(ValueError, match=match):
                ds.update_spheres(bad, c["idx"])
    finally:
        ds.close()


def test_a_bad_device_record_is_refused_alone(gpu, orc):
    """A NaN radius in a device tensor: the call reports it, the record is not stored, every other record is, and every box
    is consistent with the spheres actually stored -- the scene equals a fresh scene of the records that were applied."""
    import torch
    c = _case(gpu, orc, "general")
    ds = gpu.DeviceScene(c["scene"])
    try:
        j = len(c["idx"]) // 3
        bad = c["rec"].copy()
        bad["radius"][j] = np.nan
        applied = np.arange(len(bad)) != j
        with pytest.raises(ValueError, match="device-resident record"):
            ds.update_spheres(_tensor(bad, torch.device("cuda", ds.device)), c["idx"])
        want = rf.moved_scene(c["scene"], c["idx"][applied], c["rec"][applied])
        assert ds.spheres().tobytes() == want.spheres().tobytes()
        _, _, lo, hi = rf.refit(c["scene"], c["idx"][applied], c["rec"][applied])
        rf.same_values(_boxes(gpu, ds, 5, np.float32), rf.bound(lo, hi), "bound")
        got = _boxes(gpu, ds, 0, gpu.NODE_DTYPE)
        rf.same_values(got["bmin"], want.nodes()["bmin"], "nodes_ref bmin")
        rf.same_values(got["bmax"], want.nodes()["bmax"], "nodes_ref bmax")
        ref, cnt = orc.OracleScene.from_host(want, c["nx"], c["ny"]).render(c["ns"], seed_base=SEED)
        fb, st = ds.render(c["frame"])
        assert st.rays == cnt["rays"]
        _same(fb, ref, "after the refused record")
        bad["radius"][j] = c["rec"]["radius"][j]
        bad["mat"][j] = len(c["scene"].materials())                               # a material out of range is refused the same way
        with pytest.raises(ValueError, match="device-resident record"):
            ds.update_spheres(_tensor(bad, torch.device("cuda", ds.device)), c["idx"])
        assert ds.spheres().tobytes() == want.spheres().tobytes()
    finally:
        ds.close()


def test_refusals_leave_the_scene_alone(gpu, orc):
    c = _case(gpu, orc, "general")
    scene = c["scene"]
    ds = gpu.DeviceScene(scene)
    try:
        sph = scene.spheres()
        under = np.flatnonzero(rf.instanced(scene.instances(), len(sph)))
        fb, _ = ds.render(c["frame"])
        _same(fb, c["first"], "before")
        two = c["idx"][[0, 1, 0]]
        for rec, idx, match in ((sph[under[:1]], under[:1], "child of an instance"), (c["rec"][[0, 1, 0]], two, "twice"),
                                (c["rec"][:1], [len(sph)], "out of range"), (c["rec"][:1], [-1], "out of range")):
            with pytest.raises(ValueError, match=match):
                ds.update_spheres(rec, idx)
        nan = c["rec"][:1].copy()
        nan["c0"][0, 1] = np.inf
        with pytest.raises(ValueError, match="non-finite"):
            ds.update_spheres(nan, c["idx"][:1], recalibrate=True)
        assert gpu.rt_lib().rt_scene_update_spheres(ds._p, None, 0, 0, None) == 1
        ds.update_spheres(sph[:0])                                                # count == 0: a successful no-op
        assert ds.spheres().tobytes() == sph.tobytes()
        fb, _ = ds.render(c["frame"])
        _same(fb, c["first"], "after the refusals")
    finally:
        ds.close()


def test_a_pending_render_is_finished_with_the_old_spheres(gpu, orc):
    import torch
    c = _case(gpu, orc, "general")
    ds = gpu.DeviceScene(c["scene"])
    try:
        buf = torch.zeros((c["ny"], c["nx"], 3), dtype=torch.float32, device=torch.device("cuda", ds.device))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        ds.render(c["frame"], out=buf.data_ptr(), stream=side.cuda_stream, blocking=False)
        ds.update_spheres(c["rec"], c["idx"])
        st = ds.finish()
        side.synchronize()
        assert st.rays == c["rays0"]
        _same(buf.cpu().numpy(), c["first"], "the pending frame")
        fb, _ = ds.render(c["frame"])
        _same(fb, c["ref"], "the frame after it")
    finally:
        ds.close()


def test_multi_update_on_one_gpu(gpu, orc):
    """rt_multi_update_spheres: the multi frame after the update is the single-device frame, and so is every rank's share of a
    two-rank partition rendered on the updated scene."""
    c = _case(gpu, orc, "spheres")
    ms = gpu.MultiScene(c["scene"], 1)
    try:
        ms.update_spheres(c["rec"], c["idx"])
        fb, st = ms.render(c["frame"], tile_rows=4)
        assert st.rays == c["rays"]
        _same(fb, c["ref"], "multi")
        with pytest.raises(ValueError, match="twice"):
            ms.update_spheres(c["rec"][[0, 0]], c["idx"][[0, 0]])
    finally:
        ms.close()
    ds = gpu.DeviceScene(c["scene"])
    try:
        ds.update_spheres(c["rec"], c["idx"])
        for rank in range(2):
            f = c["scene"].frame(nx=c["nx"], ny=c["ny"], ns=c["ns"], seed_base=SEED, tile_rows=4, tile_first=rank, tile_stride=2)
            part, _ = ds.render(f)
            _same(part, c["ref"][gpu.local_rows_to_global(f)], f"rank {rank}")
    finally:
        ds.close()
