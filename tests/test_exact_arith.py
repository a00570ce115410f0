"""The cheaper exact arithmetic of the render path through the diagnostic entry rt_debug_arith_tests
(include/rt_abi.h): every mode runs a helper of csrc/rt_xorwow.h / csrc/rt_device_funcs.h and, inside the kernel, the plain
expression it replaces, and compares the two bit for bit.  The tolerance is zero everywhere: the comparison is with the
compiler's own sequence, so no reference value is needed.  (The exact division on an in-range fast path that DESIGN.md 7.4
describes was measured slower and is not in the tree; it has no mode here.)

  draws     all 2^32 words, the one-fma uniform draw and the rejection loops' signed draw 2u - 1; the identity is also run on the
            CPU (2^24 words, float32 against the float64-exact value rounded once), so that it does not rest on the GPU alone
  loose     the 65 536 tie-heavy cases of tests/test_box_tests.py (its generator, copied): the sign-folded loose_setup against
            the form with selects, clo and chi, wherever finite_inv holds
  frames    64x48 at 8 spp, kernel 3 against kernel 0 and the oracle bit for bit with equal ray counts: the random scene, book1,
            Cornell off the scan, fog, an instanced scene, and a scene whose rays have zero direction components (not admitted to the walk loop)
"""
import numpy as np
import pytest

from test_gpu_parity import assert_frames_equal, render

F = np.float32
FLT_MAX = np.finfo(np.float32).max
UNIFORM, SIGNED, LOOSE = range(3)


def run(L, mode, n, a=None, b=None, bound=None, want_path=True):
    path = np.zeros(n, np.uint8) if want_path else None
    out = np.zeros(3, np.uint64)
    st = L.rt_debug_arith_tests(mode, n, a.ctypes.data if a is not None else None, b.ctypes.data if b is not None else None,
                                bound.ctypes.data if bound is not None else None, path.ctypes.data if want_path else None, out.ctypes.data)
    assert st == 0, L.rt_last_error_detail().decode()
    if want_path:
        assert path.max() <= 1                                # every case was written
    return int(out[0]), int(out[1]), int(out[2]), path


# ------------------------------------------------------------------ draws
def test_draw_identities_on_the_cpu():
    """fma(x, 2^-32, 2^-33) is the exact sum rounded once; the exact sum fits a float64 (at most 34 significant bits), so float64
    arithmetic followed by one rounding to float32 IS the fma.  It must equal the two float32 operations of curand_uniform, and
    the doubled constants followed by - 1 must equal 2u - 1, on 2^24 words of stride 2^8 and around every power of two."""
    k = np.arange(1 << 24, dtype=np.uint64) << np.uint64(8)
    edges = np.concatenate([np.array([(1 << p) + d for d in (-2, -1, 0, 1, 2)], np.int64) for p in range(1, 33)])
    words = np.concatenate([k, edges[(edges >= 0) & (edges < (1 << 32))].astype(np.uint64)]).astype(np.uint32)
    xf = words.astype(F)                                       # (float)x: round to nearest even, as v_cvt_f32_u32
    two_ops = (xf * F(2.3283064e-10)).astype(F) + F(2.3283064e-10 / 2.0)
    assert F(2.3283064e-10) == F(2.0 ** -32) and F(2.3283064e-10) / F(2.0) == F(2.0 ** -33)
    one_fma = (xf.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(F)
    assert np.array_equal(two_ops.view(np.uint32), one_fma.view(np.uint32))
    signed_old = (F(2.0) * two_ops).astype(F) - F(1.0)
    signed_new = (xf.astype(np.float64) * 2.0 ** -31 + 2.0 ** -32).astype(F) - F(1.0)
    assert np.array_equal(signed_old.view(np.uint32), signed_new.view(np.uint32))
    assert two_ops.min() > 0.0 and two_ops.max() <= 1.0       # (0, 1]: nothing subnormal, nothing overflows


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [UNIFORM, SIGNED])
def test_draws_all_words(gpu, mode):
    mismatches, first, _, _ = run(gpu.rt_lib(), mode, 1 << 32, want_path=False)
    print("mode", mode, "words", 1 << 32, "mismatches", mismatches, "first", first if mismatches else None)
    assert mismatches == 0, (mismatches, first)


# ------------------------------------------------------------------ loose_setup: the generator of tests/test_box_tests.py, copied
N_GRID, N_SCENE, N_FLAT, N_LIMIT, N_REJECT, N_ZERO = 24576, 24576, 4096, 8192, 2048, 2048
N_CASES = N_GRID + N_SCENE + N_FLAT + N_LIMIT + N_REJECT + N_ZERO


def slab_values(bmin, bmax, o, d):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (F(1.0) / d).astype(F)
        t0 = ((bmin - o).astype(F) * inv).astype(F)
        t1 = ((bmax - o).astype(F) * inv).astype(F)
    swap = inv < F(0.0)
    return np.where(swap, t1, t0), np.where(swap, t0, t1), inv


def finite_inv_expected(o, d, bound):
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = (F(1.0) / d).astype(F)
        e = (np.abs(inv) * (np.abs(o) + bound).astype(F)).astype(F)
    return np.all(np.abs(inv) < np.inf, axis=1) & (np.max(e, axis=1) < F(1e30))


def scene_rays(rng, nodes, n, flat=False):
    pick = rng.integers(0, len(nodes), n)
    bmin, bmax = nodes["bmin"][pick].astype(F), nodes["bmax"][pick].astype(F)
    if flat:
        axis = rng.integers(0, 3, n)
        rows = np.arange(n)
        bmax[rows, axis] = bmin[rows, axis]
    size = np.maximum(bmax - bmin, F(0.05))
    target = (bmin + bmax) * F(0.5) + (rng.random((n, 3)).astype(F) - F(0.5)) * size * F(1.5)
    o = (np.array([13.0, 2.0, 3.0], F) + rng.normal(0.0, 4.0, (n, 3)).astype(F)).astype(F)
    o[:, 1] = np.abs(o[:, 1]) + F(0.01)
    d = (target - o).astype(F)
    d *= rng.uniform(0.5, 2.0, (n, 1)).astype(F)
    d[np.abs(d) < F(1e-3)] = F(1e-3)
    return bmin, bmax, o, d


def build_cases(art):
    rng = np.random.default_rng(20260919)
    hs = art.HostScene("random_scene", 1200, 800)
    nodes = hs.nodes().copy()
    hs.close()
    bound = np.maximum(np.abs(nodes["bmin"]).max(axis=0), np.abs(nodes["bmax"]).max(axis=0)).astype(F)
    parts = []

    def add(name, bmin, bmax, o, d, tmin, tmax):
        parts.append([np.ascontiguousarray(x, F) for x in (o, d)])

    # grid
    n = N_GRID
    bmin = rng.integers(-4, 5, (n, 3)).astype(F)
    thick = rng.choice(np.array([0, 1, 2, 3], F), (n, 3), p=[0.1, 0.3, 0.3, 0.3])
    bmax = bmin + thick
    d = rng.choice(np.array([-2, -1, -0.5, 0.5, 1, 2], F), (n, 3))
    through = bmin + np.floor(rng.random((n, 3)) * (2 * thick + 3) - 1).astype(F) * F(0.5)
    o = (through - rng.integers(0, 4, (n, 1)).astype(F) * F(2.0) * d).astype(F)
    near, far, _ = slab_values(bmin, bmax, o, d)
    own = np.concatenate([near, far], axis=1)[np.arange(n), rng.integers(0, 6, n)]
    kind = rng.integers(0, 4, n)
    tmax = np.select([kind == 0, kind == 1, kind == 2], [np.full(n, FLT_MAX, F), rng.integers(0, 9, n).astype(F), own], own + F(0.5))
    tmin = rng.choice(np.array([0.0, 0.001, 1.0, -1.0], F), n)
    add("grid", bmin, bmax, o, d, tmin, tmax.astype(F))
    # scene
    bmin, bmax, o, d = scene_rays(rng, nodes, N_SCENE)
    add("scene", bmin, bmax, o, d, np.full(N_SCENE, 0.001, F), np.where(rng.random(N_SCENE) < 0.5, FLT_MAX, rng.uniform(0.5, 4.0, N_SCENE)).astype(F))
    # flat
    bmin, bmax, o, d = scene_rays(rng, nodes, N_FLAT, flat=True)
    add("flat", bmin, bmax, o, d, np.full(N_FLAT, 0.001, F), np.full(N_FLAT, FLT_MAX, F))
    # limit
    n = N_LIMIT
    bmin, bmax, o, d = scene_rays(rng, nodes, n)
    near, far, _ = slab_values(bmin, bmax, o, d)
    own = np.concatenate([near, far], axis=1)[np.arange(n), rng.integers(0, 6, n)]
    add("limit", bmin, bmax, o, d, np.full(n, 0.001, F), own)
    # reject
    n = N_REJECT
    bmin, bmax, o, d = scene_rays(rng, nodes, n)
    rows, axis = np.arange(n), rng.integers(0, 3, n)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    others = np.abs(d).copy()
    others[rows, axis] = np.inf
    d[rows, axis] = (np.sign(d[rows, axis]) * others.min(axis=1) * F(1e-30)).astype(F)
    add("reject", bmin, bmax, o, d, np.full(n, 0.001, F), np.full(n, FLT_MAX, F))
    # zero
    n = N_ZERO
    bmin, bmax, o, d = scene_rays(rng, nodes, n)
    rows, axis = np.arange(n), rng.integers(0, 3, n)
    d[rows, axis] = np.where(rng.random(n) < 0.5, F(0.0), F(-0.0))
    o[rows[: n // 2], axis[: n // 2]] = bmin[rows[: n // 2], axis[: n // 2]]
    add("zero", bmin, bmax, o, d, np.full(n, 0.001, F), np.full(n, FLT_MAX, F))

    o, d = (np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(2))
    assert len(o) == N_CASES == 65536
    return o, d, bound


@pytest.mark.gpu
def test_loose_setup_sign_folded(gpu):
    o, d, bound = build_cases(gpu)
    finite = finite_inv_expected(o, d, bound)
    assert (d < 0).any(axis=1).sum() > N_CASES // 4 and finite.sum() > N_CASES // 2     # both signs of 1/d, and most rays admitted
    mismatches, first, admitted, path = run(gpu.rt_lib(), LOOSE, N_CASES, o, d, bound)
    print("loose_setup cases", N_CASES, "finite_inv", admitted, "mismatches", mismatches, "first", first if mismatches else None)
    assert np.array_equal(path.astype(bool), finite) and admitted == int(finite.sum())
    assert mismatches == 0, (mismatches, first)


# ------------------------------------------------------------------ frames
# scene: options beside the shipped ones
FRAMES = {"bouncing": {},                       # the random scene
          "book1": {},
          "cornell": {"lds_mode": 1},           # forced off the scan
          "fog": {},
          "instanced": {},
          "degenerate": {}}                     # zero direction components: the reference-form trip, no loose_setup


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FRAMES))
def test_frames_bit_for_bit(gpu, orc, name):
    nx, ny, ns = 64, 48, 8
    img, iw, ih = gpu.default_texture(name)
    hs = gpu.HostScene(name, nx, ny, img, iw, ih)
    ref, cnt = orc.OracleScene(name, nx, ny, img, iw, ih).render(ns)
    base, st0 = render(gpu, hs, 0, ns=ns)
    fb, st = render(gpu, hs, 3, FRAMES[name], ns=ns)
    assert st.kernel_variant // 1000 == 3, st.kernel_variant
    if "lds_mode" in FRAMES[name]:
        assert st.kernel_variant // 100 % 10 == FRAMES[name]["lds_mode"], st.kernel_variant
    assert st.rays == st0.rays == cnt["rays"], (name, st.rays, st0.rays, cnt["rays"])
    assert np.array_equal(fb.view(np.uint32), base.view(np.uint32)), name
    assert_frames_equal(base, ref, f"{name} kernel 0")
    assert_frames_equal(fb, ref, f"{name} kernel 3")


# (after the GPU tests on purpose: it loads the render library, and a process that loads it before torch finds no device)
def test_argument_checks_run_before_the_device(art):
    """Null pointers, an unknown mode, n out of range and a bad bound are RT_ERR_INVALID with a detail string; what passes the
    checks gets as far as the device and no further."""
    L = art.rt_lib()
    v = np.ones(3, F)
    out = np.zeros(3, np.uint64)
    path = np.zeros(1, np.uint8)
    A, O = v.ctypes.data, out.ctypes.data
    bounds = [np.array(b, F) for b in ([1, -1, 1], [1, np.inf, 1], [np.nan, 1, 1])]
    bad = [[LOOSE, 1, None, A, A, None, O], [LOOSE, 1, A, None, A, None, O], [LOOSE, 1, A, A, None, None, O], [LOOSE, 1, A, A, A, None, None],
           [UNIFORM, 1, None, None, None, None, None], [UNIFORM, 1, None, None, None, path.ctypes.data, O],
           [-1, 1, A, A, A, None, O], [3, 1, A, A, A, None, O],
           [LOOSE, 0, A, A, A, None, O], [LOOSE, (1 << 24) + 1, A, A, A, None, O], [UNIFORM, 0, None, None, None, None, O],
           [SIGNED, (1 << 32) + 1, None, None, None, None, O]]
    bad += [[LOOSE, 1, A, A, b.ctypes.data, None, O] for b in bounds]
    for args in bad:
        st = L.rt_debug_arith_tests(*args)
        text = L.rt_last_error_detail().decode()
        assert st == 1 and text.startswith("rt_debug_arith_tests:"), (args[:2], st, text)
    if art._initialised_device is None:
        assert L.rt_debug_arith_tests(LOOSE, 1, A, A, A, None, O) == 2                # RT_ERR_NO_DEVICE
