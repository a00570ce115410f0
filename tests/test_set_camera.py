"""rt_scene_set_camera on the GPU: after the call every frame entry writes, bit for bit, what it writes on a scene created with
that camera -- rt_render against the CPU oracle of the description with the camera in it, the other entries against a scene
freshly created from that description -- with and without recalibration; the cost prior changes exactly when asked to; the
original camera brings the original frame back; a pending render and a progressive state survive the change."""
import ctypes as C

import numpy as np
import pytest

import aov_expect as ax
import reproject_expect as rx
import scene_gen as sg

pytestmark = pytest.mark.gpu

SEED = 1984
DEGREES = 20.0
# a general recipe (quads, boxes, instances, media, textures) at 4 spp, and the headline random scene at 32 spp: from 32 samples
# on rt_render runs its ranked, split schedule, which is what a stale cost prior feeds
CASES = {"general": (ax.GENERAL, 48, 32, 4), "headline": ("random_scene", 96, 64, 32)}
_cache = {}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} values differ, first at {bad[:3].tolist()}"


def _case(art, orc, name):
    """The scene, its orbited camera, the description with that camera in it and the oracle's frame of it; made once."""
    if name not in _cache:
        key, nx, ny, ns = CASES[name]
        if "/" in key:
            recipe, seed = key.split("/")
            scene = sg.generate(recipe, int(seed), nx, ny)
            assert {"quad_tests", "inst_calls", "medium_calls"} <= scene.contents
            cam = rx.orbited_gen_camera(scene, nx, ny, DEGREES)
        else:
            scene = art.HostScene(key, nx, ny)
            eye = (13.0, 2.0, 3.0)                                   # host/rtw_scenes.cpp, bouncing_spheres
            cam = art.make_camera(rx.orbit(eye, (0, 0, 0), DEGREES), (0, 0, 0), (0, 1, 0), 30.0, nx / ny, 0.1, float(np.linalg.norm(eye)), 0.0, 1.0)
        moved = rx.WithCamera(art, scene, cam)
        o = orc.OracleScene.from_host(moved, nx, ny)
        ref, cnt = o.render(ns, seed_base=SEED)
        first, cnt0 = orc.OracleScene.from_host(scene, nx, ny).render(ns, seed_base=SEED)
        assert not np.array_equal(ref, first)                        # another view, not the same frame again
        _cache[name] = dict(scene=scene, cam=cam, moved=moved, ref=ref, rays=cnt["rays"], first=first, rays0=cnt0["rays"],
                            frame=scene.frame(nx=nx, ny=ny, ns=ns, seed_base=SEED), nx=nx, ny=ny, ns=ns)
    return _cache[name]


def _camera_bytes(c):
    b = bytearray(bytes(c))
    off = type(c).pad.offset
    b[off:off + 4] = b"\0" * 4
    return bytes(b)


def _cal_cost(art, ds):
    """rt_debug_cal_cost: the calibration costs the scene holds, (ny, nx) uint32 (the grid is at most 256 on its long side)."""
    nx, ny = C.c_int32(0), C.c_int32(0)
    buf = np.zeros(256 * 256, np.uint32)
    assert art.rt_lib().rt_debug_cal_cost(ds._p, buf.ctypes.data, buf.size, C.byref(nx), C.byref(ny)) == 0
    return buf[: nx.value * ny.value].reshape(ny.value, nx.value).copy()


@pytest.mark.parametrize("recalibrate", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_render_after_set_camera_equals_the_oracle(gpu, orc, name, recalibrate):
    c = _case(gpu, orc, name)
    ds = gpu.DeviceScene(c["scene"])
    try:
        info = ds.walk_info()
        ds.set_camera(c["cam"], recalibrate=recalibrate)
        assert _camera_bytes(ds.camera()) == _camera_bytes(c["cam"])             # get_camera returns what was set
        assert ds.walk_info() == info                                             # the walk array is kept
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays"] and st.samples == c["nx"] * c["ny"] * c["ns"], (st.rays, c["rays"], st.samples)
        _same(fb, c["ref"], f"{name} recalibrate={recalibrate}")
        # ... and the original camera restores the original frame
        ds.set_camera(c["scene"].desc.camera, recalibrate=recalibrate)
        fb, st = ds.render(c["frame"])
        assert st.rays == c["rays0"]
        _same(fb, c["first"], f"{name} back at the original camera")
    finally:
        ds.close()


@pytest.mark.parametrize("name", list(CASES))
def test_every_other_frame_entry_equals_a_fresh_scene(gpu, orc, name):
    """render_aov, render_aov_through, render_adaptive and render_variance after set_camera (the prior left stale) against the
    same calls on a scene created from the description with that camera."""
    c = _case(gpu, orc, name)
    ds, fresh = gpu.DeviceScene(c["scene"]), gpu.DeviceScene(c["moved"])
    try:
        ds.set_camera(c["cam"])
        f = c["frame"]
        for what, call in (("aov", lambda s: s.render_aov(f, ids=True)),
                           ("aov_through", lambda s: s.render_aov_through(f, ids=True, through=True, bounces=True))):
            got, want = call(ds), call(fresh)
            assert set(got) == set(want)
            for k in want:
                _same(got[k], want[k], f"{name} {what} {k}")
        lo = 2 if c["ns"] < 8 else c["ns"] // 4
        got, want = ds.render_adaptive(f, lo, c["ns"], 0.05), fresh.render_adaptive(f, lo, c["ns"], 0.05)
        _same(got[0], want[0], f"{name} adaptive fb")
        _same(got[1], want[1], f"{name} adaptive spp")
        assert (got[2].rays, got[2].samples) == (want[2].rays, want[2].samples)
        assert len(np.unique(want[1])) > 1                                        # pixels did stop at different checkpoints
        got, want = ds.render_variance(f, 2), fresh.render_variance(f, 2)
        _same(got[0], want[0], f"{name} variance fb")
        _same(got[1], want[1], f"{name} variance")
        _same(got[0], c["ref"], f"{name} variance fb against the oracle")
        assert (got[2].rays, got[2].samples) == (want[2].rays, want[2].samples)
    finally:
        ds.close()
        fresh.close()


def test_cost_prior_changes_only_on_recalibration(gpu, orc):
    c = _case(gpu, orc, "headline")
    ds, fresh = gpu.DeviceScene(c["scene"]), gpu.DeviceScene(c["moved"])
    try:
        before = _cal_cost(gpu, ds)
        ds.set_camera(c["cam"], recalibrate=False)
        assert np.array_equal(_cal_cost(gpu, ds), before)                              # stale
        ds.set_camera(c["cam"], recalibrate=True)
        after = _cal_cost(gpu, ds)
        assert after.shape == before.shape and not np.array_equal(after, before)
        assert np.array_equal(after, _cal_cost(gpu, fresh))                            # the grid a fresh scene measures for this camera
        tall = gpu.make_camera(rx.orbit((13.0, 2.0, 3.0), (0, 0, 0), DEGREES), (0, 0, 0), (0, 1, 0), 30.0, 0.5, 0.1, 13.5, 0.0, 1.0)
        ds.set_camera(tall, recalibrate=True)                                     # the grid's aspect comes from the new camera
        assert _cal_cost(gpu, ds).shape == (256, 128)
    finally:
        ds.close()
        fresh.close()


def test_a_pending_render_is_finished_with_its_own_camera(gpu, orc):
    """A non-blocking rt_render, then set_camera: the pending frame is the old camera's, the next one the new camera's."""
    import torch
    c = _case(gpu, orc, "general")
    ds = gpu.DeviceScene(c["scene"])
    try:
        buf = torch.zeros((c["ny"], c["nx"], 3), dtype=torch.float32, device=torch.device("cuda", ds.device))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        ds.render(c["frame"], out=buf.data_ptr(), stream=side.cuda_stream, blocking=False)
        ds.set_camera(c["cam"])
        st = ds.finish()
        side.synchronize()
        assert st.rays == c["rays0"]
        _same(buf.cpu().numpy(), c["first"], "the pending frame")
        fb, st = ds.render(c["frame"])
        _same(fb, c["ref"], "the frame after it")
    finally:
        ds.close()


def test_a_progressive_state_survives_a_camera_change(gpu, orc):
    """Windows before the change use the old camera, windows after it the new one: the first window is the old camera's frame,
    and the mixed accumulation is finite and is neither camera's frame (what it means is the caller's business)."""
    c = _case(gpu, orc, "general")
    ds = gpu.DeviceScene(c["scene"])
    try:
        pf = ds.progressive(c["frame"])
        half = c["ns"] // 2
        fb, _ = pf.render(0, half)
        want, _ = ds.render(c["scene"].frame(nx=c["nx"], ny=c["ny"], ns=half, seed_base=SEED))
        _same(fb, want, "the first window")
        ds.set_camera(c["cam"], recalibrate=True)
        fb, st = pf.render(half, c["ns"])
        assert st.rays > 0 and np.isfinite(fb).all()
        assert not np.array_equal(fb, c["first"]) and not np.array_equal(fb, c["ref"])
        pf.close()
    finally:
        ds.close()


def test_set_camera_refusals_leave_the_scene_alone(gpu, orc):
    c = _case(gpu, orc, "general")
    ds = gpu.DeviceScene(c["scene"])
    try:
        bad = gpu.RtCamera.from_buffer_copy(c["cam"])
        bad.vertical[1] = float("inf")
        with pytest.raises(ValueError, match="finite"):
            ds.set_camera(bad)
        bad = gpu.RtCamera.from_buffer_copy(c["cam"])
        bad.time0, bad.time1 = 0.75, 0.25
        with pytest.raises(ValueError, match="time1"):
            ds.set_camera(bad, recalibrate=True)
        assert gpu.rt_lib().rt_scene_set_camera(ds._p, None, 0) == 1
        assert _camera_bytes(ds.camera()) == _camera_bytes(c["scene"].desc.camera)
        fb, _ = ds.render(c["frame"])
        _same(fb, c["first"], "after the refusals")
    finally:
        ds.close()
