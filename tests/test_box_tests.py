"""The walk's three box tests (csrc/rt_device_funcs.h: slab_test, slab_test_finite, slab_test_loose) through the diagnostic entry
rt_debug_box_tests (include/rt_abi.h), against a plain float32 restatement of the reference's aabb::hit.

slab_test_finite and slab_test_loose cut the three slabs out of (tmin, tmax) with one median-of-three per axis and end.  That
is the reference's predicate exactly only if ties -- slab values equal to each other and to a limit, boxes of zero thickness --
fall the same way, so the cases are built to tie.  One launch over N_CASES <= 65536 cases:

  grid     integer boxes (thickness 0 .. 3), half-integer origins, directions from {+-0.5, +-1, +-2}^3, limits that are integers, a
           slab value of the case itself or FLT_MAX: every slab value is a small dyadic number, exact in float32
  scene    boxes of the headline scene's tree and rays from its camera region towards them (about half hit): the part the
           cap on false passes of the widened test is taken on
  flat     the same with boxes squeezed to zero thickness along one axis and rays through that plane
  limit    scene cases whose tmax is one of their own slab values
  reject   directions with one component 1e-30 of the others: loose_ok must send them to the reference's own form
  zero     directions with a zero component (1/d infinite): finite_inv must be off, slab_test must still match

Expected: slab_test == the restatement everywhere; wherever finite_inv holds slab_test_finite == slab_test and slab_test_loose
is true wherever slab_test is; on the scene part at most 1 % of the cases pass slab_test_loose and not slab_test (checked on the
CPU too, with the widened test restated, so that the inputs themselves stay under the cap for the widening in use)."""
import numpy as np
import pytest

F = np.float32
FLT_MAX = np.finfo(np.float32).max
N_GRID, N_SCENE, N_FLAT, N_LIMIT, N_REJECT, N_ZERO = 24576, 24576, 4096, 8192, 2048, 2048
N_CASES = N_GRID + N_SCENE + N_FLAT + N_LIMIT + N_REJECT + N_ZERO
FALSE_PASS_CAP = 0.01


def slab_values(bmin, bmax, o, d):
    """(b - o) * (1 / d) per axis in float32, subtraction and multiplication separate: t0, t1 as aabb::hit orders them."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (F(1.0) / d).astype(F)
        t0 = ((bmin - o).astype(F) * inv).astype(F)
        t1 = ((bmax - o).astype(F) * inv).astype(F)
    swap = inv < F(0.0)
    return np.where(swap, t1, t0), np.where(swap, t0, t1), inv


def aabb_hit(bmin, bmax, o, d, tmin, tmax):
    """aabb::hit of the reference, axis by axis with its early exits, in float32."""
    near, far, _ = slab_values(bmin, bmax, o, d)
    tmin, tmax = tmin.copy(), tmax.copy()
    alive = np.ones(len(tmin), bool)
    for a in range(3):
        tmin = np.where(near[:, a] > tmin, near[:, a], tmin)
        tmax = np.where(far[:, a] < tmax, far[:, a], tmax)
        alive &= ~(tmax <= tmin)
    return alive


def finite_inv_expected(o, d, bound):
    """inv_is_finite && loose_ok, restated (the products in float32 as the device takes them)."""
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = (F(1.0) / d).astype(F)
        e = (np.abs(inv) * (np.abs(o) + bound).astype(F)).astype(F)
    return np.all(np.abs(inv) < np.inf, axis=1) & (np.max(e, axis=1) < F(1e30))


def loose_hit(bmin, bmax, o, d, tmin, tmax, bound):
    """slab_test_loose restated for the CPU check of the cap: fma(b, x, c) as the float64 product (exact) plus c, rounded once
    to float64 and then to float32 -- the second rounding can differ from the device's fused one by an ulp, which is far inside
    the widening; this restatement sizes the inputs, the device's own flags are what the test asserts on."""
    inv = (F(1.0) / d).astype(F)
    k = F(2.0 ** -20)
    e = (k * (np.abs(inv) * (np.abs(o) + bound).astype(F)).astype(F)).astype(F)
    c = (-(o * inv).astype(F)).astype(F)
    neg = inv < F(0.0)
    clo = np.where(neg, (c + e).astype(F), (c - e).astype(F))
    chi = np.where(neg, (c - e).astype(F), (c + e).astype(F))
    v0 = (bmin.astype(np.float64) * inv.astype(np.float64) + clo.astype(np.float64)).astype(F)
    v1 = (bmax.astype(np.float64) * inv.astype(np.float64) + chi.astype(np.float64)).astype(F)
    t_in = np.maximum(np.minimum(v0, v1).max(axis=1), tmin)
    t_out = np.minimum(np.maximum(v0, v1).min(axis=1), tmax)
    return ~(t_out <= t_in)


def scene_rays(rng, nodes, n, flat=False):
    """n boxes of the tree with a ray each from the camera's side of the scene to a point in or just around the box."""
    pick = rng.integers(0, len(nodes), n)
    bmin, bmax = nodes["bmin"][pick].astype(F), nodes["bmax"][pick].astype(F)
    if flat:
        axis = rng.integers(0, 3, n)
        rows = np.arange(n)
        bmax[rows, axis] = bmin[rows, axis]
    size = np.maximum(bmax - bmin, F(0.05))
    # the target: uniform over the box blown up 1.5 times about its centre -- a good half of the rays hit
    target = (bmin + bmax) * F(0.5) + (rng.random((n, 3)).astype(F) - F(0.5)) * size * F(1.5)
    o = (np.array([13.0, 2.0, 3.0], F) + rng.normal(0.0, 4.0, (n, 3)).astype(F)).astype(F)
    o[:, 1] = np.abs(o[:, 1]) + F(0.01)
    d = (target - o).astype(F)
    d *= rng.uniform(0.5, 2.0, (n, 1)).astype(F)              # the render's directions are not unit either
    d[np.abs(d) < F(1e-3)] = F(1e-3)                          # (zero components have a part of their own)
    return bmin, bmax, o, d


def build_cases(art):
    rng = np.random.default_rng(20260919)
    hs = art.HostScene("random_scene", 1200, 800)
    nodes = hs.nodes().copy()
    hs.close()
    bound = np.maximum(np.abs(nodes["bmin"]).max(axis=0), np.abs(nodes["bmax"]).max(axis=0)).astype(F)
    parts, names = [], []

    def add(name, bmin, bmax, o, d, tmin, tmax):
        names.append((name, len(tmin)))
        parts.append([np.ascontiguousarray(x, F) for x in (bmin, bmax, o, d, tmin, tmax)])

    # grid
    n = N_GRID
    bmin = rng.integers(-4, 5, (n, 3)).astype(F)
    thick = rng.choice(np.array([0, 1, 2, 3], F), (n, 3), p=[0.1, 0.3, 0.3, 0.3])
    bmax = bmin + thick
    d = rng.choice(np.array([-2, -1, -0.5, 0.5, 1, 2], F), (n, 3))
    # the ray passes through a half-grid point in, on or next to the box, an even number of steps from its origin
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
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)        # unit length: 1e-30 of a component is then below 1e-30
    others = np.abs(d).copy()
    others[rows, axis] = np.inf
    d[rows, axis] = (np.sign(d[rows, axis]) * others.min(axis=1) * F(1e-30)).astype(F)
    add("reject", bmin, bmax, o, d, np.full(n, 0.001, F), np.full(n, FLT_MAX, F))
    # zero
    n = N_ZERO
    bmin, bmax, o, d = scene_rays(rng, nodes, n)
    rows, axis = np.arange(n), rng.integers(0, 3, n)
    d[rows, axis] = np.where(rng.random(n) < 0.5, F(0.0), F(-0.0))
    o[rows[: n // 2], axis[: n // 2]] = bmin[rows[: n // 2], axis[: n // 2]]      # half of them start ON the slab's plane: 0 * inf
    add("zero", bmin, bmax, o, d, np.full(n, 0.001, F), np.full(n, FLT_MAX, F))

    cols = [np.concatenate([p[k] for p in parts]) for k in range(6)]
    spans, at = {}, 0
    for name, cnt in names:
        spans[name] = slice(at, at + cnt)
        at += cnt
    assert at == N_CASES <= 65536
    return {"cols": cols, "bound": bound, "spans": spans}


@pytest.fixture(scope="module")
def cases(art):
    c = build_cases(art)
    bmin, bmax, o, d, tmin, tmax = c["cols"]
    c["ref"] = aabb_hit(bmin, bmax, o, d, tmin, tmax)
    c["finite"] = finite_inv_expected(o, d, c["bound"])
    return c


def test_inputs_stay_under_the_cap_on_the_cpu(cases):
    """The restated predicates on the chosen inputs: the parts do what they are for, and the widened test's false passes on the
    scene part stay under the cap for the widening in use (2^-20 |1/d| (|o| + bound))."""
    bmin, bmax, o, d, tmin, tmax = cases["cols"]
    ref, fin, sp = cases["ref"], cases["finite"], cases["spans"]
    for name in ("grid", "scene", "flat", "limit"):
        assert fin[sp[name]].all(), name
        share = ref[sp[name]].mean()
        print(name, "hit share", round(float(share), 3))
        if name == "flat":
            assert share == 0.0                               # a slab of zero thickness is never entered: tmax <= tmin on its axis
        else:
            assert 0.1 < share < 0.9, (name, share)
    assert not fin[sp["reject"]].any() and not fin[sp["zero"]].any()
    # ties are really there: grid cases where two slab values, or a slab value and a limit, coincide
    near, far, _ = slab_values(*[x[sp["grid"]] for x in (bmin, bmax, o, d)])
    t_in = np.maximum(near.max(axis=1), tmin[sp["grid"]])
    t_out = np.minimum(far.min(axis=1), tmax[sp["grid"]])
    print("grid ties t_out == t_in:", int((t_in == t_out).sum()))
    assert (t_in == t_out).sum() > 500
    s = sp["scene"]
    loose = loose_hit(bmin[s], bmax[s], o[s], d[s], tmin[s], tmax[s], cases["bound"])
    assert not (ref[s] & ~loose).any()
    false_pass = float((loose & ~ref[s]).mean())
    print("scene false passes (CPU restatement):", false_pass)
    assert false_pass <= FALSE_PASS_CAP


@pytest.mark.gpu
def test_box_tests_match_aabb_hit(gpu, cases):
    bmin, bmax, o, d, tmin, tmax = cases["cols"]
    flags = np.zeros((N_CASES, 4), np.uint8)
    L = gpu.rt_lib()
    st = L.rt_debug_box_tests(N_CASES, bmin.ctypes.data, bmax.ctypes.data, o.ctypes.data, d.ctypes.data, tmin.ctypes.data, tmax.ctypes.data,
                              cases["bound"].ctypes.data, flags.ctypes.data)
    assert st == 0, L.rt_last_error_detail().decode()
    assert flags.max() <= 1                                   # every case was written
    exact, finite, loose, fin = (flags[:, k].astype(bool) for k in range(4))
    ref, sp = cases["ref"], cases["spans"]
    for name, s in sp.items():
        print(name, "cases", s.stop - s.start, "finite_inv", int(fin[s].sum()), "slab_test", int(exact[s].sum()), "!= aabb::hit", int((exact[s] != ref[s]).sum()),
              "finite != slab_test", int((fin[s] & (finite[s] != exact[s])).sum()), "loose misses", int((fin[s] & exact[s] & ~loose[s]).sum()),
              "loose false passes", int((fin[s] & loose[s] & ~exact[s]).sum()))
    assert np.array_equal(fin, cases["finite"])
    assert np.array_equal(exact, ref)                         # slab_test is aabb::hit, zero components included
    assert np.array_equal(finite[fin], ref[fin])              # ... and so is slab_test_finite wherever the render uses it
    assert np.array_equal(finite[fin], exact[fin])
    assert not (fin & exact & ~loose).any()                   # the widened test passes wherever aabb::hit does
    assert not (fin & ref & ~loose).any()
    s = sp["scene"]
    false_pass = float((loose[s] & ~exact[s]).mean())
    print("scene false passes (device):", false_pass)
    assert false_pass <= FALSE_PASS_CAP


# (after the GPU test on purpose: it loads the render library, and a process that loads it before torch finds no device)
def test_argument_checks_run_before_the_device(art):
    """Null pointers, n out of range and a bad bound are RT_ERR_INVALID with a detail string; what passes the checks gets as far as
    the device and no further."""
    L = art.rt_lib()
    v = np.zeros(3, F)
    one = np.ones(1, F)
    flags = np.zeros(4, np.uint8)
    good = [1, v.ctypes.data, v.ctypes.data, v.ctypes.data, v.ctypes.data, one.ctypes.data, one.ctypes.data, v.ctypes.data, flags.ctypes.data]
    bad = [good[:k] + [None] + good[k + 1:] for k in range(1, 9)] + [[0] + good[1:], [(1 << 24) + 1] + good[1:]]
    bounds = [np.array(b, F) for b in ([1, -1, 1], [1, np.inf, 1], [np.nan, 1, 1])]
    bad += [good[:7] + [b.ctypes.data] + good[8:] for b in bounds]
    for args in bad:
        st = L.rt_debug_box_tests(*args)
        text = L.rt_last_error_detail().decode()
        assert st == 1 and text.startswith("rt_debug_box_tests:"), (st, text)
    if art._initialised_device is None:
        assert L.rt_debug_box_tests(*good) == 2               # RT_ERR_NO_DEVICE
