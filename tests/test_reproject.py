"""rt_reproject / reproject() / TemporalAccumulator on the GPU.  Every comparison is bit for bit against the NumPy restatement of
the contract (tests/reproject_expect.py), NaNs compared as equal: out, out_len and motion, on seeded synthetic buffers at a
size that is no multiple of the tile with every combination of guides, on the first frame, on a real pair of frames whose
reprojection is checked not to be empty, from host arrays and device tensors, on a side stream, and through the accumulator."""
import numpy as np
import pytest

import aov_expect as ax
import reproject_expect as rx
import scene_gen as sg

pytestmark = pytest.mark.gpu

NX, NY = 37, 29            # three tiles by two, neither a multiple of 16
_cache = {}


def _synthetic():
    if "synthetic" not in _cache:
        _cache["synthetic"] = rx.synthetic(NX, NY, 7)
    return _cache["synthetic"]


def _assert_same(got, want, what):
    got = np.ascontiguousarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs in other places"
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def _check(result, want, what, motion=True):
    _assert_same(result.out, want[0], what + " out")
    _assert_same(result.length, want[1], what + " out_len")
    if motion:
        _assert_same(result.motion, want[2], what + " motion")
    else:
        assert result.motion is None


@pytest.mark.parametrize("motion", [False, True])
@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("normals", [False, True])
def test_synthetic_buffers_every_combination_of_guides(gpu, normals, ids, motion):
    """Two depth planes, sky, partly covered pixels, zero history lengths, NaN and infinities in both depths; a previous camera
    a few degrees away, the same camera, and one the points are behind (a <= 0)."""
    s = _synthetic()
    kw = rx.select(s["buffers"], normals, ids)
    for name, prev in s["cams"].items():
        want = rx.reproject(cur=s["cur"], prev=prev, **kw)
        got = gpu.reproject(cur=s["cur"], prev=prev, motion=motion, **kw)
        _check(got, want, f"{name} normals={normals} ids={ids}", motion)
    tight = dict(alpha_min=0.75, depth_tol=0.0, normal_min=0.9, max_history=4.0)      # other thresholds, the ranges' ends among them
    want = rx.reproject(cur=s["cur"], prev=s["cams"]["near"], **kw, **tight)
    _check(gpu.reproject(cur=s["cur"], prev=s["cams"]["near"], motion=motion, **kw, **tight), want, "tight thresholds", motion)


def test_first_frame(gpu):
    """A null history: out == color and out_len == 1, whatever guides are given; motion needs no history."""
    s = _synthetic()
    b = s["buffers"]
    got = gpu.reproject(b["color"], b["depth"], b["alpha"], s["cur"], s["cams"]["near"], normal=b["normal"], prim=b["prim"],
                        prev_normal=b["prev_normal"], prev_prim=b["prev_prim"], motion=True)
    assert np.array_equal(got.out.view(np.uint32), b["color"].view(np.uint32))
    assert np.array_equal(got.length, np.ones((NY, NX), np.float32))
    _check(got, rx.reproject(b["color"], b["depth"], b["alpha"], s["cur"], s["cams"]["near"]), "first frame")
    assert (got.motion != 0).any()


@pytest.mark.parametrize("nx,ny", [(1, 1), (16, 16), (17, 1), (1, 33)])
def test_small_and_tile_sized_frames(gpu, nx, ny):
    s = rx.synthetic(nx, ny, 100 * nx + ny)
    for prev in s["cams"].values():
        _check(gpu.reproject(cur=s["cur"], prev=prev, motion=True, **s["buffers"]), rx.reproject(cur=s["cur"], prev=prev, **s["buffers"]), f"{nx}x{ny}")


def _real(gpu):
    """A generated scene at 64 x 48 under two cameras 4 degrees apart: the device's feature buffers of both, an 8-spp frame
    of the first as the history and a 4-spp frame of the second as the current frame."""
    if "real" not in _cache:
        nx, ny = 64, 48
        recipe, seed = ax.GENERAL.split("/")
        scene = sg.generate(recipe, int(seed), nx, ny)
        cams = [rx.orbited_gen_camera(scene, nx, ny, d) for d in (0.0, 4.0)]
        ds = gpu.DeviceScene(scene)
        try:
            aov, color = [], []
            for cam, ns in zip(cams, (8, 4)):
                ds.set_camera(cam)
                f = scene.frame(nx=nx, ny=ny, ns=ns, gamma=1.0)
                color.append(ds.render(f)[0])
                a = ds.render_aov(scene.frame(nx=nx, ny=ny, ns=4, gamma=1.0), albedo=False, ids=True)
                aov.append(a)
        finally:
            ds.close()
        kw = dict(color=color[1], depth=aov[1]["depth"], alpha=aov[1]["alpha"], normal=aov[1]["normal"], prim=aov[1]["prim"],
                  history=color[0], history_len=np.ones((ny, nx), np.float32), prev_depth=aov[0]["depth"], prev_alpha=aov[0]["alpha"],
                  prev_normal=aov[0]["normal"], prev_prim=aov[0]["prim"])
        _cache["real"] = dict(cur=cams[1], prev=cams[0], kw=kw, want=rx.reproject(cur=cams[1], prev=cams[0], **kw))
    return _cache["real"]


def test_real_frames_with_disocclusion(gpu):
    """The condition that keeps this from passing on an empty reprojection, on the restatement's output: at least half of the
    pixels find a history, and at least 1 % of the surface pixels do not (disocclusion).  Confirmed beforehand on the oracle's
    buffers (tests/aov_expect.py), where a 4 degree orbit gives 88 % and 13 %."""
    r = _real(gpu)
    out_len = r["want"][1]
    surface = r["kw"]["alpha"] >= 0.5
    found, lost = float((out_len > 1).mean()), float((out_len[surface] == 1).mean())
    print(f"history found for {found:.3f} of the pixels, lost for {lost:.3f} of the surface pixels")
    assert found >= 0.5 and lost >= 0.01
    _check(gpu.reproject(cur=r["cur"], prev=r["prev"], motion=True, **r["kw"]), r["want"], "real frames")


def test_device_tensors_and_a_side_stream(gpu):
    """Device tensors are used in place and give the host arrays' result: a blocking call, and a non-blocking one on a side
    stream followed by a synchronise; the inputs are left alone."""
    import torch
    r = _real(gpu)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in r["kw"].items()}
    got = gpu.reproject(cur=r["cur"], prev=r["prev"], motion=True, **t)
    _check(gpu.ReprojectResult(*(x.cpu().numpy() for x in got)), r["want"], "device tensors")
    ny, nx = r["want"][1].shape
    out = torch.full((ny, nx, 3), -7.0, dtype=torch.float32, device=dev)
    out_len = torch.full((ny, nx), -7.0, dtype=torch.float32, device=dev)
    motion = torch.full((ny, nx, 2), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ret = gpu.reproject(cur=r["cur"], prev=r["prev"], out=out, out_len=out_len, motion=motion, stream=side, blocking=False, **t)
    side.synchronize()
    assert ret.out is out and ret.length is out_len and ret.motion is motion
    _check(gpu.ReprojectResult(out.cpu().numpy(), out_len.cpu().numpy(), motion.cpu().numpy()), r["want"], "side stream")
    for k, v in r["kw"].items():
        assert np.array_equal(t[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(v).view(np.uint32)), k
    with pytest.raises(ValueError, match="overlaps"):
        gpu.reproject(cur=r["cur"], prev=r["prev"], out=t["history"], **t)                  # in place is refused: taps read neighbours
    with pytest.raises(ValueError):
        gpu.reproject(cur=r["cur"], prev=r["prev"], **dict(t, depth=r["kw"]["depth"]))      # mixed kinds
    d = gpu.RtReprojectDesc()
    d.nx, d.ny, d.cur, d.prev = nx, ny, r["cur"], r["prev"]
    d.color, d.depth, d.out, d.out_len = t["color"].data_ptr(), t["depth"].data_ptr(), out.data_ptr(), out_len.data_ptr()
    d.alpha = r["kw"]["alpha"].ctypes.data                                                  # host memory, declared device memory
    d.alpha_min, d.depth_tol, d.normal_min, d.max_history = 0.5, 0.05, 0.5, 32.0
    L = gpu.rt_lib()
    import ctypes as C
    assert L.rt_reproject(C.byref(d), 1, None, 1) == 1
    text = L.rt_last_error_detail().decode()
    assert text.startswith("rt_reproject") and "alpha" in text and "device memory" in text, text


def test_temporal_accumulator_equals_the_sequence_spelled_out(gpu):
    """push() over three cameras against set_camera, render, render_aov and reproject called by hand -- and the restatement."""
    nx, ny, ns = 48, 32, 4
    recipe, seed = ax.GENERAL.split("/")
    scene = sg.generate(recipe, int(seed), nx, ny)
    cams = [rx.orbited_gen_camera(scene, nx, ny, d) for d in (0.0, 3.0, 6.0)]
    frame = scene.frame(nx=nx, ny=ny, ns=ns, gamma=2.0)
    ds = gpu.DeviceScene(scene)
    try:
        acc = gpu.TemporalAccumulator(ds, frame, depth_tol=0.1)
        pushed = [(acc.push(c).copy(), acc.length.copy()) for c in cams]
        f1 = scene.frame(nx=nx, ny=ny, ns=ns, gamma=1.0)
        prev, by_hand = None, []
        for c in cams:
            ds.set_camera(c)
            color, _ = ds.render(f1)
            a = ds.render_aov(f1, albedo=False, ids=True)
            kw = dict(color=color, depth=a["depth"], alpha=a["alpha"])
            if prev is not None:
                kw.update(normal=a["normal"], prim=a["prim"], history=prev["out"], history_len=prev["len"], prev_depth=prev["a"]["depth"],
                          prev_alpha=prev["a"]["alpha"], prev_normal=prev["a"]["normal"], prev_prim=prev["a"]["prim"])
            r = gpu.reproject(cur=c, prev=c if prev is None else prev["cam"], depth_tol=0.1, **kw)
            want = rx.reproject(cur=c, prev=c if prev is None else prev["cam"], depth_tol=0.1, **kw)
            _check(r, want, "by hand", motion=False)
            prev = dict(out=r.out, len=r.length, a=a, cam=c)
            by_hand.append((r.out, r.length))
        for k, ((po, pl), (ho, hl)) in enumerate(zip(pushed, by_hand)):
            _assert_same(po, ho, f"push {k} out")
            _assert_same(pl, hl, f"push {k} length")
        assert (pushed[0][1] == 1).all() and (pushed[2][1] == 3).any() and (pushed[2][1] == 1).any()
        den = gpu.TemporalAccumulator(ds, frame, denoise=True)
        first = den.push(cams[0])
        assert first.shape == (ny, nx, 3) and np.isfinite(first).all() and not np.array_equal(first, pushed[0][0])
    finally:
        ds.close()
