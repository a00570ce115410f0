"""The cases of tests/test_filter_domain.py -- rt_denoise, rt_denoise_variance and rt_upscale over their parameter domain and on
non-finite pixels -- and, without a device, what must hold of those cases on the restatements alone (tests/denoise_expect.py,
variance_expect.py, upscale_expect.py), so that the GPU file cannot pass by never reaching what it is there for: every
expected output of the parameter domain is finite, both branches of the upscaler's "Choose" are taken, the sums that are meant
to be subnormal are, the floors that are meant to be all that is left of a denominator are, a tap 256 pixels away lies inside
the K = 8 frames, and a poisoned input pixel changes nothing beyond the reach the header names.

The case tables, the input builders and the cached expectations live here; the GPU file imports them."""
import numpy as np
import pytest

import denoise_expect as dx
import upscale_expect as ux
import variance_expect as vx

F = np.float32
FLT_MIN = np.finfo(F).tiny
_cache = {}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def differing(got, want):
    """The indices at which two float32 arrays differ: in whether the value is a NaN or, where it is none, in any bit."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.argwhere((gn != wn) | (~gn & ~wn & (bits(got) != bits(want))))


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------------------------------- rt_denoise, rt_denoise_variance
DENOISE = dict(normal_sharpness=4, sigma_depth=0.2, sigma_color=2.0, color_floor=0.01)
VARIANCE = dict(normal_sharpness=4, sigma_depth=0.2, sigma_variance=3.0, variance_floor=1e-4)
GUIDES = ("albedo", "normal", "depth")
NX, NY, K_DOMAIN = 65, 33, 4
# (nx, ny, K): taps 32, 64 and 128 pixels apart; at K = 8 the taps 256 away land inside the image one way and the other way
# crosses a workgroup tile.  They run on the "smooth" frames, where such taps carry weight.
DENOISE_FAR = [(140, 40, 6), (140, 40, 7), (260, 18, 8), (18, 260, 8)]
VARIANCE_FAR = [(140, 40, 6), (260, 18, 8)]
# name -> (input builder, the parameters that differ from DENOISE), at NX x NY and K_DOMAIN iterations
DENOISE_DOMAIN = {
    "normal_sharpness=1": ("synthetic", dict(normal_sharpness=1)),
    "normal_sharpness=10": ("synthetic", dict(normal_sharpness=10)),
    "sigma_depth=1e-6": ("flat", dict(sigma_depth=1e-6)),
    "sigma_depth=1e6": ("synthetic", dict(sigma_depth=1e6)),
    "sigma_color=1e-6": ("synthetic", dict(sigma_color=1e-6)),
    "sigma_color=1e6": ("synthetic", dict(sigma_color=1e6)),
    "color_floor=1e-45,sigma_color=1e-6": ("flat", dict(color_floor=1e-45, sigma_color=1e-6)),
    "color_floor=1e-38,sigma_color=1e-6": ("flat", dict(color_floor=1e-38, sigma_color=1e-6)),
    "color_floor=1e-45": ("flat", dict(color_floor=1e-45)),
}
DENOISE_FLOORS = [k for k in DENOISE_DOMAIN if k.startswith("color_floor")]
# name -> (input builder, the parameters that differ from VARIANCE, demodulate)
VARIANCE_DOMAIN = {
    "sigma_variance=1e-6": ("synthetic", dict(sigma_variance=1e-6), True),
    "sigma_variance=1e6": ("synthetic", dict(sigma_variance=1e6), True),
    "variance_floor=1e-45,demodulated": ("flat", dict(variance_floor=1e-45), True),
    "variance_floor=1e-45,plain": ("flat", dict(variance_floor=1e-45), False),
}
VARIANCE_FLOORS = [k for k in VARIANCE_DOMAIN if k.startswith("variance_floor")]


def frame(kind, nx, ny):
    """Seeded inputs of both filters per builder and shape (colour, the three guides and a variance); made once, left unchanged."""
    def make():
        seed = 1000 * nx + ny
        if kind == "flat":
            s = dx.synthetic_flat(nx, ny, seed)
            s["variance"] = vx.synthetic_flat_variance(nx, ny, seed)
        elif kind == "smooth":
            s = dx.synthetic_smooth(nx, ny, seed)
            s["variance"] = vx.synthetic_variance(nx, ny, seed)
        else:
            s = dx.synthetic(nx, ny, seed)
            s["variance"] = vx.synthetic_variance(nx, ny, seed)
        return s
    return _cached(("frame", kind, nx, ny), make)


def denoise_expected(kind, nx, ny, K, **params):
    s = frame(kind, nx, ny)
    kw = dict(DENOISE, iterations=K, **params)
    return _cached(("denoise", kind, nx, ny, tuple(sorted(kw.items()))), lambda: dx.denoise(s["color"], s["albedo"], s["normal"], s["depth"], **kw))


def variance_expected(kind, nx, ny, K, demodulate=True, **params):
    """(out, variance_out)"""
    s = frame(kind, nx, ny)
    kw = dict(VARIANCE, iterations=K, demodulate=demodulate, **params)
    return _cached(("variance", kind, nx, ny, tuple(sorted(kw.items()))),
                   lambda: vx.denoise_variance(s["color"], s["variance"], s["albedo"], s["normal"], s["depth"], **kw))


# ----------------------------------------------------------------------------------------------------------------- rt_upscale
UPSCALE = dict(ux.DEFAULTS)
UPSCALE_NEW_FACTORS = [(36, 18, 6), (42, 21, 7), (6, 6, 6), (7, 7, 7)]
UPSCALE_SHAPES = [(36, 18, 6), (51, 33, 3)]
# (input builder, normal_sharpness, sigma_depth, min_weight), each at both UPSCALE_SHAPES: both ends of the sharpness at each of
# three values of min_weight, and both ends of sigma_depth.  synthetic()'s jitter leaves no pixel with W >= W0 (min_weight = 1:
# every factor of every tap exactly 1), none with W >= W0 / 64 at d^1024 on the smaller shape, and none with depths equal to a
# few ulp (sigma_depth = 1e-6): those cases run on the block-constant guides, so that both branches are taken in each.
UPSCALE_DOMAIN = [("synthetic", 1, 0.2, 0.0), ("synthetic", 1, 0.2, 2.0 ** -6), ("blocks", 1, 0.2, 1.0),
                  ("synthetic", 10, 0.2, 0.0), ("blocks", 10, 0.2, 2.0 ** -6), ("blocks", 10, 0.2, 1.0),
                  ("blocks", 4, 1e-6, 2.0 ** -6), ("synthetic", 4, 1e6, 2.0 ** -6)]


def upscale_inputs(kind, nx, ny, f):
    make = ux.synthetic_blocks if kind == "blocks" else ux.synthetic
    return _cached(("upscale inputs", kind, nx, ny, f), lambda: make(nx, ny, f, ux.seed_of(nx, ny, f)))


def upscale_args(s):
    return {k: s[k] for k in ("albedo_lo", "normal_lo", "depth_lo", "albedo", "normal", "depth")}


def upscale_expected(kind, nx, ny, f, **params):
    """(out, weight_out, the mask of the guided pixels)"""
    s = upscale_inputs(kind, nx, ny, f)
    kw = dict(UPSCALE, **params)
    return _cached(("upscale", kind, nx, ny, f, tuple(sorted(kw.items()))), lambda: ux.upscale(s["color_lo"], f, weight="mask", **upscale_args(s), **kw))


# ------------------------------------------------------------------------------------------------------- poisoned inputs
VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "-1": -1.0}
# (i, j): the corner, the last pixel, a pixel on the seam of two wave tiles (x = 7 | 8), one on the seam of two workgroups (15 | 16)
POSITIONS = [(0, 0), (NX - 1, NY - 1), (7, 8), (16, 15)]
POISON_K = [2, 4]                    # reach 6 and 30; K = 4 has a direct iteration beyond the staged ones
DENOISE_PLANES = ["color", "albedo", "normal", "depth"]
VARIANCE_PLANES = DENOISE_PLANES + ["variance"]
UP_NX, UP_NY, UP_F = 68, 36, 4
UP_COARSE = ["color_lo", "albedo_lo", "normal_lo", "depth_lo"]
UP_FINE = ["albedo", "normal", "depth"]
# coarse pixels: the corner, the last one, two whose reach in the output lies across x = 7 | 8 and across x = 15 | 16, one inside
UP_COARSE_POSITIONS = [(0, 0), (UP_NX // UP_F - 1, UP_NY // UP_F - 1), (1, 1), (3, 3), (7, 4)]
UP_FINE_POSITIONS = [(0, 0), (UP_NX - 1, UP_NY - 1), (7, 8), (16, 15)]


def values_of(plane):
    """NaN and both infinities; for the planes with a domain of their own also -1: finite, outside it."""
    return ["nan", "+inf", "-inf"] + (["-1"] if plane.split("_")[0] in ("depth", "albedo", "variance") else [])


def poisoned(s, plane, n, pos, value):
    """The inputs `s` with one value of `plane` replaced, at pixel pos = (i, j); of a three-channel plane channel n mod 3."""
    t = dict(s)
    t[plane] = s[plane].copy()
    i, j = pos
    if t[plane].ndim == 3:
        t[plane][j, i, n % 3] = value
    else:
        t[plane][j, i] = value
    return t


def denoise_reach(K, plane, variance_mode=False):
    """Reach each way, a square: 2 (2^K - 1), and one more through the 3x3 pre-blur of the variance (which the albedo scales)."""
    return dx.reach(K) + (1 if variance_mode and plane in ("variance", "albedo") else 0)


def beyond(nx, ny, pos, r):
    """The mask of the pixels more than r away from pos, either way."""
    i, j = pos
    return (np.abs(np.arange(ny) - j) > r)[:, None] | (np.abs(np.arange(nx) - i) > r)[None, :]


def upscale_beyond(plane, pos):
    """The output pixels a poisoned coarse pixel Q cannot touch (those with I outside Qx - 1 .. Qx + 1 or J outside
    Qy - 1 .. Qy + 1), or a poisoned fine guide (every other pixel)."""
    if plane in UP_FINE:
        return beyond(UP_NX, UP_NY, pos, 0)
    I, J = np.arange(UP_NX) // UP_F, np.arange(UP_NY) // UP_F
    return (np.abs(J - pos[1]) > 1)[:, None] | (np.abs(I - pos[0]) > 1)[None, :]


def denoise_poisoned(K, plane, n, value):
    s = poisoned(frame("synthetic", NX, NY), plane, n, POSITIONS[n], VALUES[value])
    return s, _cached(("denoise poisoned", K, plane, n, value),
                      lambda: dx.denoise(s["color"], s["albedo"], s["normal"], s["depth"], **dict(DENOISE, iterations=K)))


def variance_poisoned(K, plane, n, value):
    s = poisoned(frame("synthetic", NX, NY), plane, n, POSITIONS[n], VALUES[value])
    return s, _cached(("variance poisoned", K, plane, n, value),
                      lambda: vx.denoise_variance(s["color"], s["variance"], s["albedo"], s["normal"], s["depth"], **dict(VARIANCE, iterations=K)))


def upscale_positions(plane):
    return UP_FINE_POSITIONS if plane in UP_FINE else UP_COARSE_POSITIONS


def upscale_poisoned(plane, n, value):
    s = poisoned(upscale_inputs("synthetic", UP_NX, UP_NY, UP_F), plane, n, upscale_positions(plane)[n], VALUES[value])
    return s, _cached(("upscale poisoned", plane, n, value), lambda: ux.upscale(s["color_lo"], UP_F, weight=True, **upscale_args(s), **UPSCALE))


# ================================================================================================================ the tests
def test_every_expected_output_of_the_denoiser_is_finite():
    for nx, ny, K in DENOISE_FAR:
        assert np.isfinite(denoise_expected("smooth", nx, ny, K)).all(), (nx, ny, K)
    for name, (kind, params) in DENOISE_DOMAIN.items():
        out = denoise_expected(kind, NX, NY, K_DOMAIN, **params)
        assert np.isfinite(out).all(), name
        assert not np.array_equal(out, denoise_expected(kind, NX, NY, K_DOMAIN)), f"{name} changes nothing"


def test_every_expected_output_of_the_variance_mode_is_finite():
    for nx, ny, K in VARIANCE_FAR:
        out, vout = variance_expected("smooth", nx, ny, K)
        assert np.isfinite(out).all() and np.isfinite(vout).all() and (vout >= 0).all(), (nx, ny, K)
    for name, (kind, params, demodulate) in VARIANCE_DOMAIN.items():
        out, vout = variance_expected(kind, NX, NY, K_DOMAIN, demodulate, **params)
        assert np.isfinite(out).all() and np.isfinite(vout).all() and (vout >= 0).all(), name
        assert not np.array_equal(out, variance_expected(kind, NX, NY, K_DOMAIN, demodulate)[0]), f"{name} changes nothing"


@pytest.mark.parametrize("nx,ny,K", [c for c in DENOISE_FAR if c[2] == 8])
def test_a_tap_256_pixels_away_lies_inside_the_frame(nx, ny, K):
    """K = 8: the last iteration's outer taps (2 s = 256) are fetched, one way; the other way every tap but the middle row or
    column is skipped."""
    s = 1 << (K - 1)
    inside = [dx._shift(np.zeros((ny, nx), F), s, ddx, ddy)[1].any() for ddx, ddy in ((2, 0), (-2, 0), (0, 2), (0, -2))]
    assert inside == ([True, True, False, False] if nx > ny else [False, False, True, True])


@pytest.mark.parametrize("nx,ny,K,variance_mode", [c + (False,) for c in DENOISE_FAR] + [c + (True,) for c in VARIANCE_FAR])
def test_the_far_taps_carry_weight(nx, ny, K, variance_mode):
    """On the frames of the far-tap cases the spacing of the last iteration matters to most of the frame: with its taps at half
    the distance, as a capped or mistaken step would place them, more than half of the values come out different."""
    s = frame("smooth", nx, ny)
    steps = [1 << k for k in range(K - 1)] + [1 << (K - 2)]
    if variance_mode:
        want = variance_expected("smooth", nx, ny, K)[0]
        near = vx.denoise_variance(s["color"], s["variance"], s["albedo"], s["normal"], s["depth"], **dict(VARIANCE, iterations=K), steps=steps)[0]
    else:
        want = denoise_expected("smooth", nx, ny, K)
        near = dx.denoise(s["color"], s["albedo"], s["normal"], s["depth"], **dict(DENOISE, iterations=K), steps=steps)
    share = len(differing(near, want)) / want.size
    print(f"{nx}x{ny} K={K}: {share:.3f} of the values depend on the last iteration's spacing")
    assert share > 0.5


def _first_denominators(name, variance_mode):
    """The 24 denominators of the colour (or variance) factor in iteration 0, over the pairs inside the image."""
    if variance_mode:
        kind, params, demodulate = VARIANCE_DOMAIN[name]
        s = frame(kind, NX, NY)
        sigma, floor = F(dict(VARIANCE, **params)["sigma_variance"]), F(dict(VARIANCE, **params)["variance_floor"])
        t = vx._variance_scale(s["albedo"]) if demodulate else F(1)
        v = vx.preblur((s["variance"] * t) * t if demodulate else s["variance"])
    else:
        kind, params = DENOISE_DOMAIN[name]
        s = frame(kind, NX, NY)
        sigma, floor = F(dict(DENOISE, **params)["sigma_color"]), F(dict(DENOISE, **params)["color_floor"])
        x = s["color"] / np.fmax(s["albedo"], dx.ALBEDO_FLOOR)
        sp = (x[..., 0] + x[..., 1]) + x[..., 2]
    dens = []
    with np.errstate(all="ignore"):
        for ddy in range(-2, 3):
            for ddx in range(-2, 3):
                if ddx or ddy:
                    q, ok = dx._shift(v if variance_mode else sp, 1, ddx, ddy)
                    den = (sigma * sigma) * (v + q) + floor if variance_mode else sigma * ((sp + q) + floor)
                    assert den.dtype == F
                    dens.append(den[ok])
    return np.concatenate(dens)


@pytest.mark.parametrize("name", DENOISE_FLOORS)
def test_colour_floor_cases_have_denominators_that_are_the_floor_alone(name):
    """Between two black pixels the colour factor's denominator is sigma_color times the floor: exactly 0 or subnormal.  A
    zero denominator makes r = 0 / 0, and max(1 - r, 0) is then 0, not a NaN: the expected frame is finite (asserted above)."""
    den = _first_denominators(name, False)
    tiny = int((den < FLT_MIN).sum())
    print(name, "pairs with a zero or subnormal denominator:", tiny, "of them zero:", int((den == 0).sum()))
    assert tiny >= 20 and (den >= 0).all()


@pytest.mark.parametrize("name", VARIANCE_FLOORS)
def test_variance_floor_cases_have_denominators_that_are_the_floor_alone(name):
    """Between two pixels of zero (pre-blurred) variance the denominator is the subnormal floor; inside the flat region the
    colours are equal as well, so r = 0 / floor = 0 and the tap is fully kept.  A flushed floor would make it 0 / 0."""
    den = _first_denominators(name, True)
    tiny = int((den < FLT_MIN).sum())
    print(name, "pairs with a subnormal denominator:", tiny)
    assert tiny >= 20 and (den > 0).all()
    kind, params, demodulate = VARIANCE_DOMAIN[name]
    s = frame(kind, NX, NY)
    _, (j0, j1, i0, i1) = dx.flat_regions(NX, NY)
    x = s["color"] / np.fmax(s["albedo"], dx.ALBEDO_FLOOR) if demodulate else s["color"]
    assert (bits(x[j0:j1, i0:i1]) == bits(x[j0, i0])).all() and (s["variance"][j0:j1, i0:i1] == 0).all()


@pytest.mark.parametrize("kind,m,sigma_depth,min_weight", UPSCALE_DOMAIN)
@pytest.mark.parametrize("nx,ny,f", UPSCALE_SHAPES)
def test_upscaler_cases_take_both_branches(nx, ny, f, kind, m, sigma_depth, min_weight):
    """At least 5 % of the pixels take each branch of "Choose" -- the guided one alone at min_weight = 0, where the plain spline
    is left for W = 0 exactly -- and the expected frame is finite."""
    out, wout, guided = upscale_expected(kind, nx, ny, f, normal_sharpness=m, sigma_depth=sigma_depth, min_weight=min_weight)
    share = guided.mean()
    print(f"{kind} {nx}x{ny} f={f} m={m} sigma_depth={sigma_depth} min_weight={min_weight}: guided {share:.3f}")
    assert np.isfinite(out).all() and np.isfinite(wout).all()
    assert share >= 0.05
    if min_weight > 0:
        assert 1 - share >= 0.05
    else:
        assert np.array_equal(guided, wout > 0)


@pytest.mark.parametrize("nx,ny,f", UPSCALE_SHAPES)
def test_sharpness_10_leaves_subnormal_weight_sums(nx, ny, f):
    """normal_sharpness = 10, min_weight = 0: d^1024 is subnormal for d near 0.92, and with no free centre tap all nine weights
    of a pixel can be: at least 20 guided pixels have 0 < W < FLT_MIN, where W > 0 decides the branch and the result is a
    quotient of two subnormals.  Counted where W / W0 = weight_out is subnormal: W0 <= 1 up to rounding, so W is too."""
    out, wout, guided = upscale_expected("synthetic", nx, ny, f, normal_sharpness=10, sigma_depth=0.2, min_weight=0.0)
    tiny = guided & (wout > 0) & (wout < FLT_MIN)          # W <= W / W0 up to rounding
    print(f"{nx}x{ny} f={f}: guided pixels with a subnormal W: {int(tiny.sum())}")
    assert tiny.sum() >= 20
    assert np.isfinite(out[tiny]).all()


@pytest.mark.parametrize("nx,ny,f", UPSCALE_SHAPES)
def test_jittered_guides_leave_nothing_at_the_smallest_sigma_depth(nx, ny, f):
    """Why the sigma_depth = 1e-6 case has a builder of its own: synthetic()'s 2 % depth jitter kills every tap."""
    assert not upscale_expected("synthetic", nx, ny, f, sigma_depth=1e-6)[2].any()
    counts = np.sort(np.unique(upscale_inputs("blocks", nx, ny, f)["depth"], return_counts=True)[1])[::-1]
    assert counts[:12].sum() >= 0.85 * nx * ny              # the blocks builder: a dozen depths at most hold nearly every pixel


def test_new_factor_shapes_are_in_the_upscaler_table():
    assert all(s in ux.SHAPES for s in UPSCALE_NEW_FACTORS)
    B7, _ = ux.spline_weights(7, 7)
    exact = ((2 * np.arange(7) + 1) / 14.0 - 0.5)
    assert (B7[1].astype(np.float64) != 0.75 - exact * exact).any()      # factor 7: the weights are rounded


# ---- (b) on the restatement: the reach formulae
def _check_reach(got, clean, far, what, touched=None):
    bad = differing(got, clean)
    outside = [tuple(b) for b in bad if far[b[0], b[1]]]
    assert not outside, f"{what}: {len(outside)} values beyond reach differ from the clean frame, first at {outside[:3]}"
    if touched is not None:
        assert len(bad) >= touched, f"{what}: only {len(bad)} values differ from the clean frame"


@pytest.mark.parametrize("plane", DENOISE_PLANES)
@pytest.mark.parametrize("K", POISON_K)
def test_denoise_restatement_keeps_a_poisoned_pixel_within_reach(K, plane):
    clean = denoise_expected("synthetic", NX, NY, K)
    for n, pos in enumerate(POSITIONS):
        far = beyond(NX, NY, pos, denoise_reach(K, plane))
        assert far.any()
        for value in values_of(plane):
            _, out = denoise_poisoned(K, plane, n, value)
            _check_reach(out, clean, far, f"K={K} {plane} {value} at {pos}", touched=1 if plane == "color" else None)
            if plane == "color":          # the formula is tight: a NaN in the colour is felt at the edge of the square
                bad = differing(out, clean)
                r = dx.reach(K)
                assert np.abs(bad[:, 1] - pos[0]).max() == min(r, max(pos[0], NX - 1 - pos[0]))
                assert np.abs(bad[:, 0] - pos[1]).max() == min(r, max(pos[1], NY - 1 - pos[1]))


@pytest.mark.parametrize("plane", VARIANCE_PLANES)
@pytest.mark.parametrize("K", POISON_K)
def test_variance_restatement_keeps_a_poisoned_pixel_within_reach(K, plane):
    clean, clean_v = variance_expected("synthetic", NX, NY, K)
    for n, pos in enumerate(POSITIONS):
        far = beyond(NX, NY, pos, denoise_reach(K, plane, True))
        assert far.any()
        for value in values_of(plane):
            _, (out, vout) = variance_poisoned(K, plane, n, value)
            _check_reach(out, clean, far, f"K={K} {plane} {value} at {pos}")
            _check_reach(vout, clean_v, far, f"K={K} {plane} {value} at {pos}: variance_out", touched=1 if plane == "variance" else None)
            if plane == "variance" and value == "nan":     # tight: the pre-blur carries it one pixel further than the taps
                bad = differing(vout, clean_v)
                r = dx.reach(K) + 1
                assert np.abs(bad[:, 1] - pos[0]).max() == min(r, max(pos[0], NX - 1 - pos[0]))


@pytest.mark.parametrize("plane", UP_COARSE + UP_FINE)
def test_upscale_restatement_keeps_a_poisoned_pixel_within_reach(plane):
    clean, clean_w, _ = upscale_expected("synthetic", UP_NX, UP_NY, UP_F)
    for n, pos in enumerate(upscale_positions(plane)):
        far = upscale_beyond(plane, pos)
        assert far.any() and not far.all()
        for value in values_of(plane):
            _, (out, wout) = upscale_poisoned(plane, n, value)
            _check_reach(out, clean, far, f"{plane} {value} at {pos}", touched=1 if plane == "color_lo" else None)
            _check_reach(wout, clean_w, far, f"{plane} {value} at {pos}: weight_out")
            if plane == "color_lo" and value == "nan":      # tight: every output pixel with a tap on Q is touched
                assert np.isnan(out).any(axis=2)[~far].all()
