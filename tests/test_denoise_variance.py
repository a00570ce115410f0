"""rt_denoise_variance / denoise(variance=...) / DeviceScene.render_denoised(variance=True) on the GPU.  Every comparison is bit
for bit against the NumPy float32 restatement of the contract (tests/variance_expect.py): frame shapes smaller than a tile,
ragged and of several tiles each way, iteration counts on both sides of the staged / direct switch, each value of the option,
the guides on and off, demodulation, in place, the workspace and stream rules, host arrays, and the whole pipeline."""
import numpy as np
import pytest

import aov_expect as ax
import denoise_expect as dx
import variance_expect as vx

pytestmark = pytest.mark.gpu

PARAMS = dict(normal_sharpness=4, sigma_depth=0.2, sigma_variance=3.0, variance_floor=1e-4)
SHAPES = [(1, 1), (5, 3), (37, 29), (65, 33)]
_cache = {}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _inputs(nx, ny):
    """Seeded inputs per shape; made once, left unchanged."""
    if (nx, ny) not in _cache:
        s = dx.synthetic(nx, ny, 1000 * nx + ny)
        s["variance"] = vx.synthetic_variance(nx, ny, 1000 * nx + ny)
        _cache[nx, ny] = s
    return _cache[nx, ny]


def _expect(nx, ny, guides=("albedo", "normal", "depth"), **kw):
    key = (nx, ny, tuple(guides), tuple(sorted(kw.items())))
    if key not in _cache:
        s = _inputs(nx, ny)
        _cache[key] = vx.denoise_variance(s["color"], s["variance"], **{g: s[g] for g in guides}, **kw)
    return _cache[key]


def _assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_shapes_and_iterations(gpu, nx, ny, K):
    """K = 5 reaches the direct variant (taps 8 and 16 apart); the variance input is 0 in places."""
    s = _inputs(nx, ny)
    vout = np.full((ny, nx), -7.0, np.float32)
    got = gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], iterations=K, variance=s["variance"], variance_out=vout, **PARAMS)
    want, wantv = _expect(nx, ny, iterations=K, **PARAMS)
    _assert_same(got, want, f"{nx}x{ny} K={K}")
    _assert_same(vout, wantv, f"{nx}x{ny} K={K} variance_out")


@pytest.mark.parametrize("lds", [-1, 0, 1])
@pytest.mark.parametrize("nx,ny", [(37, 29), (65, 33)])
def test_every_option_gives_the_same_frame(gpu, nx, ny, lds):
    """denoise_lds: auto, direct everywhere, staged up to taps 8 apart (K = 5 covers both sides of each switch)."""
    s = _inputs(nx, ny)
    vout = np.empty((ny, nx), np.float32)
    try:
        gpu.set_option("denoise_lds", lds)
        got = gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], iterations=5, variance=s["variance"], variance_out=vout, **PARAMS)
    finally:
        gpu.reset_options()
    want, wantv = _expect(nx, ny, iterations=5, **PARAMS)
    _assert_same(got, want, f"denoise_lds={lds}")
    _assert_same(vout, wantv, f"denoise_lds={lds} variance_out")


@pytest.mark.parametrize("guides", [("albedo", "normal", "depth"), ("albedo",), ("normal", "depth"), ()])
def test_guides_on_and_off(gpu, guides):
    """65 x 33, K = 4 (three staged iterations and a direct one): every guide on; normal and depth off; demodulation off; all
    off -- the four kernel specialisations a guide set selects, in both variants."""
    s = _inputs(65, 33)
    vout = np.empty((33, 65), np.float32)
    got = gpu.denoise(s["color"], **{g: s[g] for g in guides}, iterations=4, variance=s["variance"], variance_out=vout, **PARAMS)
    want, wantv = _expect(65, 33, guides, iterations=4, **PARAMS)
    _assert_same(got, want, f"guides {guides}")
    _assert_same(vout, wantv, f"guides {guides} variance_out")
    for one in (("albedo", "normal"), ("albedo", "depth")):
        got = gpu.denoise(s["color"], **{g: s[g] for g in one}, iterations=4, variance=s["variance"], **PARAMS)
        _assert_same(got, _expect(65, 33, one, iterations=4, **PARAMS)[0], f"guides {one}")


def test_device_tensors_workspace_streams_in_place_and_host(gpu):
    """Device tensors are used in place: a caller's workspace with blocking=False on a side stream (then synchronize), a null
    workspace without variance_out, out = color, and the same frame from host arrays in place."""
    import torch
    nx, ny = 65, 33
    s = _inputs(nx, ny)
    want, wantv = _expect(nx, ny, iterations=5, **PARAMS)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
    ws = torch.empty(gpu.denoise_workspace_bytes(nx, ny), dtype=torch.uint8, device=dev)
    out = torch.full((ny, nx, 3), -7.0, dtype=torch.float32, device=dev)
    vout = torch.full((ny, nx), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ret = gpu.denoise(t["color"], t["albedo"], t["normal"], t["depth"], iterations=5, out=out, workspace=ws, stream=side, blocking=False,
                      variance=t["variance"], variance_out=vout, **PARAMS)
    side.synchronize()
    assert ret is out
    _assert_same(out.cpu().numpy(), want, "caller workspace, side stream")
    _assert_same(vout.cpu().numpy(), wantv, "caller workspace, side stream: variance_out")
    for k in ("color", "variance"):
        assert np.array_equal(_bits(t[k].cpu().numpy()), _bits(s[k]))                          # the inputs are left alone
    made = gpu.denoise(t["color"], t["albedo"], t["normal"], t["depth"], iterations=5, variance=t["variance"], **PARAMS)
    _assert_same(made.cpu().numpy(), want, "null workspace, no variance_out")
    same = gpu.denoise(t["color"], t["albedo"], t["normal"], t["depth"], iterations=5, out=t["color"], workspace=ws, stream=side.cuda_stream,
                       variance=t["variance"], **PARAMS)
    assert same is t["color"]
    _assert_same(t["color"].cpu().numpy(), want, "in place")
    host, hv = s["color"].copy(), np.empty((ny, nx), np.float32)
    gpu.denoise(host, s["albedo"], s["normal"], s["depth"], iterations=5, out=host, variance=s["variance"], variance_out=hv, **PARAMS)
    _assert_same(host, want, "host arrays in place")
    _assert_same(hv, wantv, "host arrays: variance_out")
    with pytest.raises(ValueError):
        gpu.denoise(t["color"], variance=s["variance"], iterations=1, **PARAMS)                 # mixed kinds
    with pytest.raises(ValueError, match="variance_out"):
        gpu.denoise(t["color"], variance=t["variance"], variance_out=t["variance"], iterations=1, **PARAMS)


def test_render_denoised_with_variance(gpu, orc):
    """The whole pipeline at 32 x 24: "noisy" and "variance" are render_variance's, the features render_aov's, and "color" is the
    expectation fed with those device buffers."""
    c = ax.Case(gpu, orc, ax.GENERAL)
    ds = gpu.DeviceScene(c.scene)
    try:
        f = c.scene.frame(nx=32, ny=24, ns=8, gamma=2.0, seed_base=ax.SEED)
        r = ds.render_denoised(f, variance=True, iterations=3)
        assert set(r) == {"color", "noisy", "albedo", "normal", "depth", "variance"}
        f1 = c.scene.frame(nx=32, ny=24, ns=8, gamma=1.0, seed_base=ax.SEED)
        noisy, _ = ds.render(f1)
        _assert_same(r["noisy"], noisy, "noisy")
        fb, var, _ = ds.render_variance(f1, 8)
        _assert_same(r["variance"], var, "variance")
        assert (var > 0).any()
        aov = ds.render_aov(f1, alpha=False)
        for k in ("albedo", "normal", "depth"):
            _assert_same(r[k], aov[k], k)
        want, _ = vx.denoise_variance(noisy, var, aov["albedo"], aov["normal"], aov["depth"],
                                      **dict(iterations=3, normal_sharpness=4, sigma_depth=0.2, **vx.DEFAULTS))
        _assert_same(r["color"], want, "expectation")
        r4 = ds.render_denoised(f, variance=True, batches=4, iterations=3)
        _assert_same(r4["variance"], ds.render_variance(f1, 4)[1], "variance at B = 4")
    finally:
        ds.close()
