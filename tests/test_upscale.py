"""rt_upscale / upscale() / DeviceScene.render_upscaled on the GPU.  Every comparison is bit for bit against the NumPy float32
restatement of the contract (tests/upscale_expect.py): output shapes around a wave tile, a workgroup tile and the image edge
at factors that do and do not divide the tile, every subset of guides with and without demodulation, weight_out, both ends
of min_weight, each value of the option, the stream rules, host arrays against device tensors, the refusals, render_upscaled,
and a call beside a pending render."""
import ctypes as C

import numpy as np
import pytest

import aov_expect as ax
import upscale_expect as ux

pytestmark = pytest.mark.gpu

PARAMS = dict(ux.DEFAULTS)
GUIDES = ("albedo", "normal", "depth")
_cache = {}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _inputs(nx, ny, f):
    """Seeded inputs per shape; made once, left unchanged."""
    if (nx, ny, f) not in _cache:
        _cache[nx, ny, f] = ux.synthetic(nx, ny, f, ux.seed_of(nx, ny, f))
    return _cache[nx, ny, f]


def _args(s, guides=GUIDES):
    """The keyword arguments of upscale() for a subset of guides: each one on both grids."""
    kw = {}
    for g in guides:
        kw[g], kw[g + "_lo"] = s[g], s[g + "_lo"]
    return kw


def _expect(nx, ny, f, guides=GUIDES, **kw):
    """(out, weight_out) of the restatement, cached."""
    key = (nx, ny, f, tuple(guides), tuple(sorted(kw.items())))
    if key not in _cache:
        s = _inputs(nx, ny, f)
        _cache[key] = ux.upscale(s["color_lo"], f, weight=True, **_args(s, guides), **kw)
    return _cache[key]


def _assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


@pytest.mark.parametrize("nx,ny,f", ux.SHAPES)
def test_shapes_and_factors(gpu, nx, ny, f):
    """One coarse pixel (eight taps skipped), one coarse column, one coarse row, an image smaller than a wave tile, one coarse
    pixel past a wave tile and past a workgroup tile, factors that do not divide the tile, the largest factor."""
    s = _inputs(nx, ny, f)
    weight = np.full((ny, nx), -7.0, np.float32)
    got = gpu.upscale(s["color_lo"], f, weight_out=weight, **_args(s), **PARAMS)
    want, want_w = _expect(nx, ny, f, **PARAMS)
    _assert_same(got, want, f"{nx}x{ny} f={f}")
    _assert_same(weight, want_w, f"{nx}x{ny} f={f} weight_out")


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("depth_on", [False, True])
@pytest.mark.parametrize("normal_on", [False, True])
@pytest.mark.parametrize("nx,ny,f", [(130, 66, 2), (85, 45, 5)])
def test_every_subset_of_guides(gpu, nx, ny, f, normal_on, depth_on, demodulate):
    """Each of the four kernel specialisations, with and without demodulation.  A guide is turned off by leaving its buffers
    out."""
    s = _inputs(nx, ny, f)
    guides = (("albedo",) if demodulate else ()) + (("normal",) if normal_on else ()) + (("depth",) if depth_on else ())
    weight = np.empty((ny, nx), np.float32)
    got = gpu.upscale(s["color_lo"], f, weight_out=weight, **_args(s, guides), **PARAMS)
    want, want_w = _expect(nx, ny, f, guides, **PARAMS)
    _assert_same(got, want, f"guides {guides}")
    _assert_same(weight, want_w, f"guides {guides} weight_out")


def test_a_guide_is_also_off_by_its_parameter(gpu):
    """normal_sharpness = 0 / sigma_depth = 0 with the buffers present equal the buffers left out; albedos given with
    demodulate=False are not used."""
    nx, ny, f = 85, 45, 5
    s = _inputs(nx, ny, f)
    kw = dict(PARAMS, normal_sharpness=0, sigma_depth=0.0)
    got = gpu.upscale(s["color_lo"], f, demodulate=False, **_args(s), **kw)
    _assert_same(got, _expect(nx, ny, f, (), **kw)[0], "guides off by parameter")
    one = gpu.upscale(s["color_lo"], f, **_args(s), **dict(PARAMS, normal_sharpness=0))
    _assert_same(one, _expect(nx, ny, f, ("albedo", "depth"), **PARAMS)[0], "normal off by parameter")
    other = gpu.upscale(s["color_lo"], f, **_args(s), **dict(PARAMS, sigma_depth=0.0))
    _assert_same(other, _expect(nx, ny, f, ("albedo", "normal"), **PARAMS)[0], "depth off by parameter")


@pytest.mark.parametrize("min_weight", [0.0, 1.0])
def test_both_ends_of_min_weight(gpu, min_weight):
    """0: guided wherever any weight is left; 1: the plain spline wherever a factor took any away."""
    nx, ny, f = 51, 33, 3
    s = _inputs(nx, ny, f)
    kw = dict(PARAMS, min_weight=min_weight)
    weight = np.empty((ny, nx), np.float32)
    got = gpu.upscale(s["color_lo"], f, weight_out=weight, **_args(s), **kw)
    want, want_w = _expect(nx, ny, f, **kw)
    _assert_same(got, want, f"min_weight={min_weight}")
    _assert_same(weight, want_w, f"min_weight={min_weight} weight_out")


@pytest.mark.parametrize("lds", [-1, 0, 1])
def test_every_option_gives_the_same_frame(gpu, lds):
    """upscale_lds: auto, every tap through L1/L2, the window staged in LDS -- with every guide and with none, at a factor that
    divides the tile and at one that does not."""
    try:
        gpu.set_option("upscale_lds", lds)
        got = {}
        for nx, ny, f in [(130, 66, 2), (195, 99, 3)]:
            s = _inputs(nx, ny, f)
            got[nx, ny, f, GUIDES] = gpu.upscale(s["color_lo"], f, **_args(s), **PARAMS)
            got[nx, ny, f, ()] = gpu.upscale(s["color_lo"], f, **PARAMS)
    finally:
        gpu.reset_options()
    for (nx, ny, f, guides), frame in got.items():
        _assert_same(frame, _expect(nx, ny, f, guides, **PARAMS)[0], f"upscale_lds={lds} {nx}x{ny} f={f} guides {guides}")


def test_device_tensors_streams_and_host_arrays(gpu):
    """Device tensors are used in place and left unchanged: blocking=False on a side stream (then synchronize), out made by the
    call, and the same frame from host arrays."""
    import torch
    nx, ny, f = 136, 72, 8
    s = _inputs(nx, ny, f)
    want, want_w = _expect(nx, ny, f, **PARAMS)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
    out = torch.full((ny, nx, 3), -7.0, dtype=torch.float32, device=dev)
    weight = torch.full((ny, nx), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ret = gpu.upscale(t["color_lo"], f, out=out, weight_out=weight, stream=side, blocking=False, **_args(t), **PARAMS)
    side.synchronize()
    assert ret is out
    _assert_same(out.cpu().numpy(), want, "side stream")
    _assert_same(weight.cpu().numpy(), want_w, "side stream weight_out")
    for k, v in s.items():
        assert np.array_equal(_bits(t[k].cpu().numpy()), _bits(v)), k                          # the inputs are left alone
    made = gpu.upscale(t["color_lo"], f, stream=side.cuda_stream, **_args(t), **PARAMS)         # out made, blocking
    assert made.device == t["color_lo"].device
    _assert_same(made.cpu().numpy(), want, "out made by the call")
    before = {k: v.copy() for k, v in s.items()}
    host = gpu.upscale(s["color_lo"], f, **_args(s), **PARAMS)                                  # host arrays
    _assert_same(host, want, "host arrays")
    for k, v in s.items():
        assert np.array_equal(_bits(before[k]), _bits(v)), k


def test_refusals(gpu):
    """A host pointer passed as device memory, out overlapping albedo, a CPU tensor and mixed kinds: nothing is launched."""
    import torch
    nx, ny, f = 6, 4, 2
    s = _inputs(nx, ny, f)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
    out = torch.full((ny, nx, 3), -7.0, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        gpu.upscale(t["color_lo"], f, albedo_lo=s["albedo_lo"], albedo=t["albedo"], **PARAMS)      # mixed
    with pytest.raises(ValueError):
        gpu.upscale(torch.from_numpy(s["color_lo"]), f, **PARAMS)                                   # a CPU tensor
    with pytest.raises(ValueError, match="out overlaps"):
        gpu.upscale(t["color_lo"], f, out=t["albedo"], **_args(t), **PARAMS)                        # out is albedo
    d = gpu.RtUpscaleDesc()
    d.nx, d.ny, d.factor, d.normal_sharpness, d.sigma_depth, d.min_weight = nx, ny, f, 4, 0.2, 2.0 ** -6
    d.color_lo, d.out = t["color_lo"].data_ptr(), out.data_ptr()
    d.depth_lo, d.depth = t["depth_lo"].data_ptr(), s["depth"].ctypes.data                          # host memory, declared device memory
    L = gpu.rt_lib()
    assert L.rt_upscale(C.byref(d), 1, None, 1) == 1
    text = L.rt_last_error_detail().decode()
    assert text.startswith("rt_upscale: ") and "depth" in text and "device memory" in text, text
    d.depth = t["depth"].data_ptr()
    d.albedo, d.out = t["albedo"].data_ptr(), t["albedo"].data_ptr() + 12                          # out overlaps albedo
    assert L.rt_upscale(C.byref(d), 1, None, 1) == 1
    text = L.rt_last_error_detail().decode()
    assert text.startswith("rt_upscale: ") and "out overlaps" in text, text
    assert (out.cpu().numpy() == -7.0).all()                                                        # nothing was launched
    assert np.array_equal(_bits(t["albedo"].cpu().numpy()), _bits(s["albedo"]))


@pytest.mark.parametrize("denoise", [False, True])
@pytest.mark.parametrize("factor", [2, 4])
def test_render_upscaled(gpu, orc, factor, denoise):
    """On one aov_expect scene at 32 x 24: "low" is render() at gamma 1 of the coarse frame (denoise() of it with the coarse
    guides when denoising), and "color" is the restatement applied to "low", the coarse guides and the returned guides."""
    nx, ny, ns = 32, 24, 4
    c = _cache.get("case")
    if c is None:
        c = _cache["case"] = ax.Case(gpu, orc, ax.GENERAL)
    ds = gpu.DeviceScene(c.scene)
    try:
        f = c.scene.frame(nx=nx, ny=ny, ns=ns, gamma=2.0, seed_base=ax.SEED)
        r = ds.render_upscaled(f, factor, denoise=denoise, denoise_iterations=3, min_weight=0.05)
        assert set(r) == {"color", "low", "albedo", "normal", "depth", "weight"} | ({"noisy_low"} if denoise else set())
        lo = c.scene.frame(nx=nx // factor, ny=ny // factor, ns=ns, gamma=1.0, seed_base=ax.SEED)
        noisy, _ = ds.render(lo)
        g_lo = ds.render_aov(lo, alpha=False)
        low = gpu.denoise(noisy, g_lo["albedo"], g_lo["normal"], g_lo["depth"], iterations=3) if denoise else noisy
        _assert_same(r["low"], low, "low")
        if denoise:
            _assert_same(r["noisy_low"], noisy, "noisy_low")
        g = ds.render_aov(c.scene.frame(nx=nx, ny=ny, ns=ns, gamma=1.0, seed_base=ax.SEED), alpha=False)
        for k in GUIDES:
            _assert_same(r[k], g[k], k)
        want, want_w = ux.upscale(r["low"], factor, g_lo["albedo"], g_lo["normal"], g_lo["depth"], r["albedo"], r["normal"], r["depth"], weight=True,
                                  **dict(ux.DEFAULTS, min_weight=0.05))
        _assert_same(r["color"], want, "color")
        _assert_same(r["weight"], want_w, "weight")
        assert r["color"].shape == (ny, nx, 3) and np.isfinite(r["color"]).all()
    finally:
        ds.close()


def test_upscale_beside_a_pending_render(gpu):
    """A non-blocking render on one stream and an upscale on another: both give their standalone results."""
    import torch
    nx, ny, f = 130, 66, 2
    s = _inputs(nx, ny, f)
    want, _ = _expect(nx, ny, f, **PARAMS)
    hs = gpu.HostScene("bouncing", ax.NX, ax.NY)
    ds = gpu.DeviceScene(hs)
    try:
        frame = hs.frame(nx=ax.NX, ny=ax.NY, ns=64)
        ref_fb, ref_st = ds.render(frame)
        dev = torch.device("cuda", ds.device)
        buf = torch.zeros((ax.NY, ax.NX, 3), dtype=torch.float32, device=dev)
        t = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
        out = torch.zeros((ny, nx, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        ds.render(frame, out=buf.data_ptr(), stream=sa.cuda_stream, blocking=False)
        gpu.upscale(t["color_lo"], f, out=out, stream=sb, blocking=False, **_args(t), **PARAMS)
        sb.synchronize()
        st = ds.finish()
        sa.synchronize()
        assert st.rays == ref_st.rays
        assert np.array_equal(_bits(buf.cpu().numpy()), _bits(ref_fb))
        _assert_same(out.cpu().numpy(), want, "beside a render")
    finally:
        ds.close()
