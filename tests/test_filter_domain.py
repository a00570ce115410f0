"""rt_denoise, rt_denoise_variance and rt_upscale on the GPU over the parameter domain their argument checks admit, and on
non-finite and out-of-domain pixels.  Every comparison is bit for bit against the NumPy float32 restatements of the contracts
(tests/denoise_expect.py, variance_expect.py, upscale_expect.py); where an input holds a NaN or an infinity, the masks of the
NaNs are compared, and the bits wherever the value is no NaN.  The cases, their inputs and the cached expectations are those of
tests/test_filter_domain_host.py, which asserts on the restatements alone that the cases reach what they are there for.

The parameter domain: iterations 6 to 8 (taps up to 128 pixels apart, on frames wide enough to fetch them), upscale factors 6
and 7, both ends of normal_sharpness, of every sigma and of min_weight, the smallest floors (subnormals) on frames with exactly
black pixels and exactly zero variances, and the upscaler's weight sums in the subnormal range.  Non-finite pixels: one value
of one input plane at a time -- a NaN, an infinity of either sign, -1 where the plane has a domain -- at the image corner, the
last pixel and on the seams of the wave tiles and of the workgroups: the call succeeds, nothing beyond the contract's reach
differs from the clean frame, the staged and the direct variants agree, and the frame is the restatement's."""
import numpy as np
import pytest

import test_filter_domain_host as fd

pytestmark = pytest.mark.gpu


def _assert_same(got, want, what):
    """Bit for bit; NaNs are compared as NaNs (their sign and payload are not part of any contract)."""
    bad = fd.differing(got, want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def _assert_bits(got, want, what):
    assert not np.isnan(want).any(), what
    _assert_same(got, want, what)


# ------------------------------------------------------------------------------------------------------ the parameter domain
@pytest.mark.parametrize("lds", [-1, 0, 1])
@pytest.mark.parametrize("nx,ny,K", fd.DENOISE_FAR)
def test_denoise_far_taps(gpu, nx, ny, K, lds):
    """Iterations 6, 7 and 8 -- taps 32, 64 and 128 pixels apart -- on frames in which the far taps are fetched, not skipped,
    and carry weight."""
    s = fd.frame("smooth", nx, ny)
    try:
        gpu.set_option("denoise_lds", lds)
        got = gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], iterations=K, **fd.DENOISE)
    finally:
        gpu.reset_options()
    _assert_bits(got, fd.denoise_expected("smooth", nx, ny, K), f"{nx}x{ny} K={K} denoise_lds={lds}")


def test_denoise_eight_iterations_in_place(gpu):
    """K = 8 with out = color and a caller's workspace: the two images of the workspace swap eight times."""
    import torch
    nx, ny, K = 260, 18, 8
    s = fd.frame("smooth", nx, ny)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(s[k]).to(dev) for k in ("color",) + fd.GUIDES}
    ws = torch.empty(gpu.denoise_workspace_bytes(nx, ny), dtype=torch.uint8, device=dev)
    same = gpu.denoise(t["color"], t["albedo"], t["normal"], t["depth"], iterations=K, out=t["color"], workspace=ws, **fd.DENOISE)
    assert same is t["color"]
    _assert_bits(t["color"].cpu().numpy(), fd.denoise_expected("smooth", nx, ny, K), "K=8 in place")


@pytest.mark.parametrize("name", list(fd.DENOISE_DOMAIN))
def test_denoise_parameter_extremes(gpu, name):
    """65 x 33, K = 4: both ends of normal_sharpness, sigma_depth and sigma_color, and subnormal colour floors on a frame with
    exactly black pixels, where the denominator is 0 or subnormal and the expected frame is finite all the same."""
    kind, params = fd.DENOISE_DOMAIN[name]
    s = fd.frame(kind, fd.NX, fd.NY)
    got = gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], iterations=fd.K_DOMAIN, **dict(fd.DENOISE, **params))
    _assert_bits(got, fd.denoise_expected(kind, fd.NX, fd.NY, fd.K_DOMAIN, **params), name)


@pytest.mark.parametrize("nx,ny,K", fd.VARIANCE_FAR)
def test_variance_far_taps(gpu, nx, ny, K):
    s = fd.frame("smooth", nx, ny)
    vout = np.full((ny, nx), -7.0, np.float32)
    got = gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], iterations=K, variance=s["variance"], variance_out=vout, **fd.VARIANCE)
    want, want_v = fd.variance_expected("smooth", nx, ny, K)
    _assert_bits(got, want, f"{nx}x{ny} K={K}")
    _assert_bits(vout, want_v, f"{nx}x{ny} K={K} variance_out")


@pytest.mark.parametrize("name", list(fd.VARIANCE_DOMAIN))
def test_variance_parameter_extremes(gpu, name):
    """65 x 33, K = 4: both ends of sigma_variance; the smallest variance_floor on regions of zero variance and equal colours,
    demodulated and not, where the factor is 0 / floor = 0 -> 1 and a flushed floor would make it 0 / 0."""
    kind, params, demodulate = fd.VARIANCE_DOMAIN[name]
    s = fd.frame(kind, fd.NX, fd.NY)
    vout = np.full((fd.NY, fd.NX), -7.0, np.float32)
    got = gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], iterations=fd.K_DOMAIN, variance=s["variance"], variance_out=vout,
                      demodulate=demodulate, **dict(fd.VARIANCE, **params))
    want, want_v = fd.variance_expected(kind, fd.NX, fd.NY, fd.K_DOMAIN, demodulate, **params)
    _assert_bits(got, want, name)
    _assert_bits(vout, want_v, f"{name} variance_out")


@pytest.mark.parametrize("lds", [0, 1])
@pytest.mark.parametrize("nx,ny,f", fd.UPSCALE_NEW_FACTORS)
def test_upscale_factors_6_and_7(gpu, nx, ny, f, lds):
    """Factors 6 and 7 (7: spline weights that are not exact in binary32), direct and staged; the smallest frames have one
    coarse pixel."""
    s = fd.upscale_inputs("synthetic", nx, ny, f)
    weight = np.full((ny, nx), -7.0, np.float32)
    try:
        gpu.set_option("upscale_lds", lds)
        got = gpu.upscale(s["color_lo"], f, weight_out=weight, **fd.upscale_args(s), **fd.UPSCALE)
    finally:
        gpu.reset_options()
    want, want_w, _ = fd.upscale_expected("synthetic", nx, ny, f)
    _assert_bits(got, want, f"{nx}x{ny} f={f} upscale_lds={lds}")
    _assert_bits(weight, want_w, f"{nx}x{ny} f={f} upscale_lds={lds} weight_out")


@pytest.mark.parametrize("kind,m,sigma_depth,min_weight", fd.UPSCALE_DOMAIN)
@pytest.mark.parametrize("nx,ny,f", fd.UPSCALE_SHAPES)
def test_upscale_parameter_extremes(gpu, nx, ny, f, kind, m, sigma_depth, min_weight):
    """Both ends of normal_sharpness at three values of min_weight, and both ends of sigma_depth.  At sharpness 10 and
    min_weight 0 dozens of pixels have a subnormal W: W > 0 decides the branch and the result is a quotient of subnormals."""
    s = fd.upscale_inputs(kind, nx, ny, f)
    params = dict(normal_sharpness=m, sigma_depth=sigma_depth, min_weight=min_weight)
    weight = np.full((ny, nx), -7.0, np.float32)
    got = gpu.upscale(s["color_lo"], f, weight_out=weight, **fd.upscale_args(s), **params)
    want, want_w, _ = fd.upscale_expected(kind, nx, ny, f, **params)
    _assert_bits(got, want, f"{kind} {nx}x{ny} f={f} {params}")
    _assert_bits(weight, want_w, f"{kind} {nx}x{ny} f={f} {params} weight_out")


# ------------------------------------------------------------------------------------- non-finite and out-of-domain pixels
def _beyond_reach(got, clean, far, what):
    """(b): every value beyond reach is the clean run's expectation, bit for bit."""
    bad = [tuple(b) for b in fd.differing(got, clean) if far[b[0], b[1]]]
    assert not bad, f"{what}: {len(bad)} values beyond reach differ from the clean frame, first at {bad[:3]}"


def _denoise_variants(gpu, call):
    """The frame(s) of `call` with denoise_lds at -1 (shipped: staged up to taps 4 apart), 0 (direct) and 1 (staged up to 8)."""
    out = {}
    try:
        for lds in (-1, 0, 1):
            gpu.set_option("denoise_lds", lds)
            out[lds] = call()                                      # (a): it returns, RT_OK -- the binding raises on anything else
    finally:
        gpu.reset_options()
    return out


@pytest.mark.parametrize("plane", fd.DENOISE_PLANES)
@pytest.mark.parametrize("K", fd.POISON_K)
def test_denoise_poisoned_pixel(gpu, K, plane):
    clean = fd.denoise_expected("synthetic", fd.NX, fd.NY, K)
    for n, pos in enumerate(fd.POSITIONS):
        far = fd.beyond(fd.NX, fd.NY, pos, fd.denoise_reach(K, plane))
        for value in fd.values_of(plane):
            what = f"K={K} {plane} {value} at {pos}"
            s, want = fd.denoise_poisoned(K, plane, n, value)
            got = _denoise_variants(gpu, lambda: gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], iterations=K, **fd.DENOISE))
            _beyond_reach(got[-1], clean, far, what)                                        # (b)
            _assert_same(got[0], got[1], f"{what}: direct against staged")                 # (c)
            _assert_same(got[-1], got[0], f"{what}: shipped against direct")
            _assert_same(got[-1], want, f"{what}: against the restatement")                # (d)


@pytest.mark.parametrize("plane", fd.VARIANCE_PLANES)
@pytest.mark.parametrize("K", fd.POISON_K)
def test_variance_poisoned_pixel(gpu, K, plane):
    clean = fd.variance_expected("synthetic", fd.NX, fd.NY, K)
    for n, pos in enumerate(fd.POSITIONS):
        far = fd.beyond(fd.NX, fd.NY, pos, fd.denoise_reach(K, plane, True))
        for value in fd.values_of(plane):
            what = f"K={K} {plane} {value} at {pos}"
            s, want = fd.variance_poisoned(K, plane, n, value)

            def call():
                vout = np.full((fd.NY, fd.NX), -7.0, np.float32)
                out = gpu.denoise(s["color"], s["albedo"], s["normal"], s["depth"], iterations=K, variance=s["variance"], variance_out=vout, **fd.VARIANCE)
                return out, vout
            got = _denoise_variants(gpu, call)
            for c, name in enumerate(("out", "variance_out")):
                _beyond_reach(got[-1][c], clean[c], far, f"{what}: {name}")
                _assert_same(got[0][c], got[1][c], f"{what}: {name}, direct against staged")
                _assert_same(got[-1][c], got[0][c], f"{what}: {name}, shipped against direct")
                _assert_same(got[-1][c], want[c], f"{what}: {name} against the restatement")


@pytest.mark.parametrize("plane", fd.UP_COARSE + fd.UP_FINE)
def test_upscale_poisoned_pixel(gpu, plane):
    clean = fd.upscale_expected("synthetic", fd.UP_NX, fd.UP_NY, fd.UP_F)
    for n, pos in enumerate(fd.upscale_positions(plane)):
        far = fd.upscale_beyond(plane, pos)
        for value in fd.values_of(plane):
            what = f"{plane} {value} at {pos}"
            s, want = fd.upscale_poisoned(plane, n, value)
            got = {}
            try:
                for lds in (0, 1):
                    gpu.set_option("upscale_lds", lds)
                    weight = np.full((fd.UP_NY, fd.UP_NX), -7.0, np.float32)
                    got[lds] = (gpu.upscale(s["color_lo"], fd.UP_F, weight_out=weight, **fd.upscale_args(s), **fd.UPSCALE), weight)
            finally:
                gpu.reset_options()
            for c, name in enumerate(("out", "weight_out")):
                _beyond_reach(got[1][c], clean[c], far, f"{what}: {name}")
                _assert_same(got[0][c], got[1][c], f"{what}: {name}, direct against staged")
                _assert_same(got[1][c], want[c], f"{what}: {name} against the restatement")
