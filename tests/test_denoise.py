"""rt_denoise / denoise() / DeviceScene.render_denoised on the GPU.  Every comparison is bit for bit against the NumPy float32
restatement of the contract (tests/denoise_expect.py): frame shapes around a wave tile, a workgroup tile and the image edge,
iteration counts on both sides of the staged / direct switch, every subset of guides, demodulation, in place, the workspace
and stream rules, host arrays against device tensors, each value of the option, the refusals, render_denoised, and a call
beside a pending render."""
import ctypes as C

import numpy as np
import pytest

import aov_expect as ax
import denoise_expect as dx

pytestmark = pytest.mark.gpu

PARAMS = dict(sigma_color=2.0, color_floor=0.01, normal_sharpness=4, sigma_depth=0.2)
_cache = {}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _inputs(nx, ny):
    """Seeded inputs per shape; made once, left unchanged."""
    if (nx, ny) not in _cache:
        _cache[nx, ny] = dx.synthetic(nx, ny, 1000 * nx + ny)
    return _cache[nx, ny]


def _expect(nx, ny, guides=("albedo", "normal", "depth"), **kw):
    key = (nx, ny, tuple(guides), tuple(sorted(kw.items())))
    if key not in _cache:
        s = _inputs(nx, ny)
        _cache[key] = dx.denoise(s["color"], **{g: s[g] for g in guides}, **kw)
    return _cache[key]


def _assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 70), (70, 1), (5, 3), (63, 17), (65, 33)])
def test_shapes_and_iterations(gpu, nx, ny, K):
    """One pixel, one column, one row, an image smaller than the stencil, one pixel short of and one past a wave tile and a
    workgroup tile; K = 5 reaches the direct variant (taps 8 and 16 apart)."""
    s = _inputs(nx, ny)
    got = gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], iterations=K, **PARAMS)
    _assert_same(got, _expect(nx, ny, iterations=K, **PARAMS), f"{nx}x{ny} K={K}")


def test_halo_larger_than_a_tile(gpu):
    """80 x 48 at K = 5: the last iteration's taps are 32 pixels away, two workgroup tiles."""
    s = _inputs(80, 48)
    got = gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], iterations=5, **PARAMS)
    _assert_same(got, _expect(80, 48, iterations=5, **PARAMS), "80x48 K=5")


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("color_on", [False, True])
@pytest.mark.parametrize("depth_on", [False, True])
@pytest.mark.parametrize("normal_on", [False, True])
def test_every_subset_of_guides(gpu, normal_on, depth_on, color_on, demodulate):
    """65 x 33, K = 4 (three staged iterations and a direct one): each of the eight kernel specialisations in both variants,
    with and without demodulation.  A guide is turned off by leaving its buffer out."""
    s = _inputs(65, 33)
    guides = (("albedo",) if demodulate else ()) + (("normal",) if normal_on else ()) + (("depth",) if depth_on else ())
    kw = dict(PARAMS, iterations=4, sigma_color=2.0 if color_on else 0.0)
    got = gpu.denoise(s["color"], **{g: s[g] for g in guides}, **kw)
    _assert_same(got, _expect(65, 33, guides, **kw), f"guides {guides} colour {color_on}")


def test_a_guide_is_also_off_by_its_parameter(gpu):
    """normal_sharpness = 0 / sigma_depth = 0 with the buffers present equal the buffers left out; albedo given with
    demodulate=False is not used."""
    s = _inputs(65, 33)
    kw = dict(PARAMS, iterations=3, normal_sharpness=0, sigma_depth=0.0)
    got = gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], demodulate=False, **kw)
    _assert_same(got, _expect(65, 33, (), **kw), "guides off by parameter")


@pytest.mark.parametrize("lds", [-1, 0, 1])
def test_every_option_gives_the_same_frame(gpu, lds):
    """denoise_lds: auto, direct everywhere, staged up to taps 8 apart (K = 5 covers both sides of each switch)."""
    s = _inputs(80, 48)
    try:
        gpu.set_option("denoise_lds", lds)
        got = gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], iterations=5, **PARAMS)
        few = gpu.denoise(s["color"], iterations=4, **dict(PARAMS, sigma_color=0.0))      # the smallest LDS image: colour records only
    finally:
        gpu.reset_options()
    _assert_same(got, _expect(80, 48, iterations=5, **PARAMS), f"denoise_lds={lds}")
    _assert_same(few, _expect(80, 48, (), iterations=4, **dict(PARAMS, sigma_color=0.0)), f"denoise_lds={lds}, no guides")


def test_device_tensors_workspace_streams_and_in_place(gpu):
    """Device tensors are used in place: a caller's workspace with blocking=False on a side stream (then synchronize), a null
    workspace, out = color, and the same frame from host arrays."""
    import torch
    nx, ny = 65, 33
    s = _inputs(nx, ny)
    want = _expect(nx, ny, iterations=5, **PARAMS)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
    ws = torch.empty(gpu.denoise_workspace_bytes(nx, ny), dtype=torch.uint8, device=dev)
    out = torch.full((ny, nx, 3), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ret = gpu.denoise(t["color"], t["albedo"], t["normal"], t["depth"], iterations=5, out=out, workspace=ws, stream=side, blocking=False, **PARAMS)
    side.synchronize()
    assert ret is out
    _assert_same(out.cpu().numpy(), want, "caller workspace, side stream")
    assert np.array_equal(_bits(t["color"].cpu().numpy()), _bits(s["color"]))              # the inputs are left alone
    made = gpu.denoise(t["color"], t["albedo"], t["normal"], t["depth"], iterations=5, **PARAMS)   # null workspace, out made
    _assert_same(made.cpu().numpy(), want, "null workspace")
    same = gpu.denoise(t["color"], t["albedo"], t["normal"], t["depth"], iterations=5, out=t["color"], workspace=ws, stream=side.cuda_stream, **PARAMS)
    assert same is t["color"]
    _assert_same(t["color"].cpu().numpy(), want, "in place")
    host = s["color"].copy()
    gpu.denoise(host, s["albedo"], s["normal"], s["depth"], iterations=5, out=host, **PARAMS)         # host arrays, in place
    _assert_same(host, want, "host arrays in place")


def test_refusals(gpu):
    """A too-small workspace, a host pointer passed as device memory, a CPU tensor and mixed kinds."""
    import torch
    nx, ny = 16, 8
    s = _inputs(nx, ny)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
    small = torch.empty(gpu.denoise_workspace_bytes(nx, ny) - 16, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="workspace"):
        gpu.denoise(t["color"], workspace=small, iterations=1, **PARAMS)
    with pytest.raises(ValueError):
        gpu.denoise(t["color"], albedo=s["albedo"], iterations=1, **PARAMS)                 # mixed
    with pytest.raises(ValueError):
        gpu.denoise(torch.from_numpy(s["color"]), iterations=1, **PARAMS)                   # a CPU tensor
    d = gpu.RtDenoiseDesc()
    d.nx, d.ny, d.color, d.out = nx, ny, t["color"].data_ptr(), t["color"].data_ptr()
    d.depth = s["depth"].ctypes.data                                                        # host memory, declared device memory
    d.iterations, d.normal_sharpness, d.sigma_color, d.color_floor, d.sigma_depth = 1, 4, 2.0, 0.01, 0.2
    L = gpu.rt_lib()
    assert L.rt_denoise(C.byref(d), 1, None, 1) == 1
    text = L.rt_last_error_detail().decode()
    assert text.startswith("rt_denoise") and "depth" in text and "device memory" in text, text
    assert np.array_equal(_bits(t["color"].cpu().numpy()), _bits(s["color"]))              # nothing was launched


def test_render_denoised(gpu, orc):
    """On one aov_expect scene: "noisy" is render() at gamma 1, the features are render_aov's at min(ns, 16) samples, and
    "color" is denoise() of them -- which, these being the oracle's frames bit for bit, is the expectation on the oracle's."""
    c = ax.Case(gpu, orc, ax.GENERAL)
    ds = gpu.DeviceScene(c.scene)
    try:
        f = c.scene.frame(nx=ax.NX, ny=ax.NY, ns=4, gamma=2.0, seed_base=ax.SEED)
        r = ds.render_denoised(f, iterations=3)
        assert set(r) == {"color", "noisy", "albedo", "normal", "depth"}
        f1 = c.scene.frame(nx=ax.NX, ny=ax.NY, ns=4, gamma=1.0, seed_base=ax.SEED)
        noisy, _ = ds.render(f1)
        _assert_same(r["noisy"], noisy, "noisy")
        again = gpu.denoise(r["noisy"], r["albedo"], r["normal"], r["depth"], iterations=3)
        _assert_same(r["color"], again, "color")
        e = c.expect(4)
        for k in ("albedo", "normal", "depth"):
            _assert_same(r[k], e[k], k)
        _assert_same(r["color"], dx.denoise(noisy, e["albedo"], e["normal"], e["depth"], **dict(dx.DEFAULTS, iterations=3)), "expectation")
        with pytest.raises(ValueError):
            ds.render_denoised(c.scene.frame(nx=ax.NX, ny=ax.NY, ns=4, tile_rows=4, tile_first=1, tile_stride=3))
    finally:
        ds.close()


def test_denoise_beside_a_pending_render(gpu):
    """A non-blocking render on one stream and a denoise on another: both give their standalone results."""
    import torch
    nx, ny = 80, 48
    s = _inputs(nx, ny)
    want = _expect(nx, ny, iterations=5, **PARAMS)
    hs = gpu.HostScene("bouncing", ax.NX, ax.NY)
    ds = gpu.DeviceScene(hs)
    try:
        frame = hs.frame(nx=ax.NX, ny=ax.NY, ns=64)
        ref_fb, ref_st = ds.render(frame)
        dev = torch.device("cuda", ds.device)
        buf = torch.zeros((ax.NY, ax.NX, 3), dtype=torch.float32, device=dev)
        t = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
        out = torch.zeros((ny, nx, 3), dtype=torch.float32, device=dev)
        ws = torch.empty(gpu.denoise_workspace_bytes(nx, ny), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        ds.render(frame, out=buf.data_ptr(), stream=sa.cuda_stream, blocking=False)
        gpu.denoise(t["color"], t["albedo"], t["normal"], t["depth"], iterations=5, out=out, workspace=ws, stream=sb, blocking=False, **PARAMS)
        sb.synchronize()
        st = ds.finish()
        sa.synchronize()
        assert st.rays == ref_st.rays
        assert np.array_equal(_bits(buf.cpu().numpy()), _bits(ref_fb))
        _assert_same(out.cpu().numpy(), want, "beside a render")
    finally:
        ds.close()
