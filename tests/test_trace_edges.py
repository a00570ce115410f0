"""rt_trace_rays against the oracle's trace entry point on caller rays of every kind (trace_families): arbitrary origins,
directions and times, rays aimed at edges, silhouettes and box corners, zero direction components, extreme scales, window
edges and non-finite rays -- on every scene, every option, closest hit, any hit and hit records."""
import numpy as np
import pytest

import trace_families as tf

pytestmark = pytest.mark.gpu

SCENES = ["two_spheres", "degenerate", "bouncing", "book1", "cornell", "cornell_smoke", "final", "checker", "earth", "perlin",
          "quads", "simple_light", "original", "instanced", "fog", "crowd_4096", "crowd_4097", "crowd_2400",
          "crowd_big"]
NX, NY, NS = 48, 32, 4
OPTIONS = [(lds, tree) for lds in (0, 1, 2, -1) for tree in (0, 1)]


@pytest.fixture(scope="module")
def scenes(gpu, orc):
    cache = {}

    def get(name):
        if name not in cache:
            img, iw, ih = gpu.default_texture(name)
            hs = gpu.HostScene(name, NX, NY, img, iw, ih)
            os_ = orc.OracleScene(name, NX, NY, img, iw, ih)
            rays = tf.ray_sample(orc, os_, NX, NY, NS)
            fam = tf.families(hs, rays, lambda b: os_.trace(b.o, b.d, b.tm, b.tmin, b.tmax)[0])
            cache[name] = (hs, gpu.DeviceScene(hs), os_, fam)
        return cache[name]
    yield get
    for _, ds, _, _ in cache.values():
        ds.close()


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _trace(ds, b, **kw):
    return ds.trace(b.o, b.d, b.tm, tmin=b.tmin, tmax=b.tmax, **kw)


def _expected(os_, b):
    """The oracle's answer with the product's rule for non-finite rays applied (a miss)."""
    t, p, n, uv, mat = os_.trace(b.o, b.d, b.tm, b.tmin, b.tmax)
    bad = tf.expected_nonfinite_miss(b)
    t[bad] = tf.FLT_MAX
    p[bad], n[bad], uv[bad], mat[bad] = 0, 0, 0, -1
    return t, p, n, uv, mat


def _batches(fam, names):
    for f in names:
        for k, b in enumerate(fam[f]):
            yield f, k, b


def _check_mat_bijection(pairs):
    """(oracle material index, product material index) over all hits: a one-to-one map."""
    pairs = np.unique(np.asarray(pairs).reshape(-1, 2), axis=0)
    assert len(np.unique(pairs[:, 0])) == len(pairs) and len(np.unique(pairs[:, 1])) == len(pairs), pairs


@pytest.mark.parametrize("name", SCENES)
def test_closest_and_any_match_oracle(scenes, name):
    """Closest hit: t and hit / miss equal the oracle's bit for bit on every family; any hit equals the oracle's hit / miss.
    Non-finite rays (and the zero direction, which both sides miss on their own) are misses."""
    hs, ds, os_, fam = scenes(name)
    for f, k, b in _batches(fam, tf.FINITE_FAMILIES + ["nonfinite"]):
        t = _expected(os_, b)[0]
        r = _trace(ds, b)
        h = _trace(ds, b, any_hit=True)
        bad = np.flatnonzero(r.t.view(np.uint32) != t.view(np.uint32))
        assert len(bad) == 0, (f"{name} {f}[{k}]: {len(bad)} of {len(t)} differ; first {bad[:4]}: gpu {r.t[bad[:4]]} "
                               f"oracle {t[bad[:4]]}; o {b.o[bad[:2]]} d {b.d[bad[:2]]} tm {b.tm[bad[:2]]} tmin {b.tmin}")
        assert np.array_equal(r.prim >= 0, t < tf.FLT_MAX), (name, f, k)
        assert (r.inst[r.prim < 0] == -1).all()
        assert np.array_equal(h, t < tf.FLT_MAX), (name, f, k, np.flatnonzero(h != (t < tf.FLT_MAX))[:5])


@pytest.mark.parametrize("name", SCENES)
def test_records_match_oracle(scenes, name):
    """record=True: point, normal and uv equal the oracle's bit for bit (both sides evaluate the reference's expressions with
    the same contractions, and acos / atan2 correctly rounded); materials map one-to-one; inst is -1 exactly when the hit
    primitive is not reached through an instance.

    One exception, the sign of a zero: a quad's u or v of exactly 0 (a ray aimed at the edge) comes out -0 on one side and
    +0 on the other.  cross() is -fma(a.x, b.z, -(a.z b.x)) in its y component, and the compiler may evaluate that negated
    fma as fma(-a.x, b.z, a.z b.x), which is the same number except for the sign of an exact zero.  No later operation
    sees the difference (u and v only index textures), so those fields are compared after adding +0, which maps -0 to +0
    and changes no other bit pattern."""
    hs, ds, os_, fam = scenes(name)
    inst_tab = hs.instances()
    under = set()                                     # (kind, index) of every sphere / quad that lives under an instance
    bx = tf.boxes(hs)
    for rec in inst_tab:
        c = int(rec["child"])
        kind, idx = (c & 0xFFFFFFFF) >> 28, c & 0x0FFFFFFF
        if kind == tf.PRIM_BOX:
            under.update((tf.PRIM_QUAD, (int(bx[idx]) & 0x3FFFFFFF) + f) for f in range(6))
        else:
            under.add((kind, idx))
    pairs = []
    for f, k, b in _batches(fam, tf.FINITE_FAMILIES + ["nonfinite"]):
        t, p, n, uv, mat = _expected(os_, b)
        r = _trace(ds, b, record=True)
        plain = _trace(ds, b)
        assert _same(r.t, plain.t) and np.array_equal(r.prim, plain.prim) and np.array_equal(r.inst, plain.inst)
        assert _same(r.t, t), (name, f, k)
        for what, x, y in (("point", r.point, p), ("normal", r.normal, n), ("uv", r.uv + np.float32(0), uv + np.float32(0))):
            bad = np.flatnonzero((x.view(np.uint32) != y.view(np.uint32)).any(1))
            assert len(bad) == 0, f"{name} {f}[{k}] {what}: {len(bad)} differ, first {bad[:3]}: {x[bad[:3]]} vs {y[bad[:3]]}"
        hit = r.prim >= 0
        assert (r.mat[~hit] == -1).all() and (mat[~hit] == -1).all()
        pairs.append(np.stack([mat[hit], r.mat[hit]], 1))
        kind, idx = tf_kind(r.prim[hit]), r.prim[hit].astype(np.int64) & 0x0FFFFFFF
        inst_expected = np.array([(int(a), int(c)) in under for a, c in zip(kind, idx)], bool)
        assert np.array_equal(r.inst[hit] >= 0, inst_expected), (name, f, k)
        if len(inst_tab):
            ch = inst_tab["child"][r.inst[hit][r.inst[hit] >= 0]]
            assert (ch >= 0).all()
    _check_mat_bijection(np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int32))


def tf_kind(prim):
    return (np.asarray(prim).astype(np.int64) & 0xFFFFFFFF) >> 28


@pytest.mark.parametrize("name", SCENES)
def test_every_option_on_every_family(gpu, scenes, name):
    """All eight (trace_lds, trace_tree) settings give identical t / prim / inst on every family, non-finite rays included."""
    hs, ds, os_, fam = scenes(name)
    batches = list(_batches(fam, tf.FINITE_FAMILIES + ["nonfinite"]))
    results = []
    try:
        for lds, tree in OPTIONS:
            gpu.set_option("trace_lds", lds)
            gpu.set_option("trace_tree", tree)
            results.append([_trace(ds, b) for _, _, b in batches])
    finally:
        gpu.reset_options()
    for o, res in enumerate(results[1:], 1):
        for (f, k, _), x, y in zip(batches, results[0], res):
            assert _same(x.t, y.t) and np.array_equal(x.prim, y.prim) and np.array_equal(x.inst, y.inst), (name, OPTIONS[o], f, k)


@pytest.mark.parametrize("name", SCENES)
def test_window_rules(scenes, name):
    """Every window batch: spheres tmin < t < tmax, quads tmin <= t <= tmax, media tmin <= t and t at most two ulp above
    tmax, an empty window (tmax < tmin; with tmax == tmin a quad at t == tmin may still be hit) is a miss, and tmax = +inf
    gives the default window.

    A medium clamps its interval to [tmin, tmax] but returns t1 + hit_distance / |d| (constant_medium.cuh), which does not
    depend on tmax: its exact value is at most t2 <= tmax, and the division and the addition round once each, so t may
    land up to two ulp above tmax (the window family's tmax one ulp below a medium hit reaches exactly that).  The oracle
    does the same (test_closest_and_any_match_oracle)."""
    hs, ds, os_, fam = scenes(name)
    for k, b in enumerate(fam["window"]):
        r = _trace(ds, b)
        hit = r.prim >= 0
        tmax = np.full(len(b.o), tf.FLT_MAX, np.float32) if b.tmax is None else b.tmax
        sph = hit & (tf_kind(r.prim) == 0)
        med = hit & (tf_kind(r.prim) == 4)
        quad = hit & ~sph & ~med
        up2 = np.nextafter(np.nextafter(tmax, np.float32(np.inf)), np.float32(np.inf))
        assert (r.t[sph] > b.tmin).all() and (r.t[sph] < tmax[sph]).all(), (name, k)
        assert (r.t[quad] >= b.tmin).all() and (r.t[quad] <= tmax[quad]).all(), (name, k)
        assert (r.t[med] >= b.tmin).all() and (r.t[med] <= up2[med]).all(), (name, k)
        empty = tmax < np.float32(b.tmin)
        assert not hit[empty].any(), (name, k)
        if b.tmax is not None and np.isposinf(b.tmax).all():
            d = ds.trace(b.o, b.d, b.tm, tmin=b.tmin)
            assert _same(d.t, r.t) and np.array_equal(d.prim, r.prim)


@pytest.mark.parametrize("name", [s for s in SCENES if s not in ("cornell_smoke", "final", "original", "fog")])
def test_float64_on_gpu_output(scenes, name):
    """The solid scenes' GPU answers pass the float64 brute force directly (reported hit on its primitive, no clear hit
    missed), with the reported primitive and instance."""
    hs, ds, os_, fam = scenes(name)
    for f in ["volume", "render", "axis", "aimed"]:
        for k, b in enumerate(fam[f]):
            rows = 300 if name.startswith("crowd") else 3000    # (the brute force is O(rays x primitives))
            b = tf.Batch(*(x[:rows] if isinstance(x, np.ndarray) else x for x in b))
            r = _trace(ds, b)
            res = tf.f64_check(hs, b, r.t, r.prim, r.inst)
            assert len(res.off_surface) == 0, (name, f, k, res.off_surface[:5])
            assert len(res.missed) == 0, (name, f, k, res.missed[:5])


@pytest.mark.parametrize("name", ["bouncing", "cornell", "final", "cornell_smoke"])
def test_record_mode_batch_edges(scenes, name):
    """Record mode, where a wave finishes its rays together: batches of 1, 63, 64, 65, 255, 256, 257 and 1000 rays with hits
    and misses give the full batch's per-ray results."""
    hs, ds, os_, fam = scenes(name)
    b = fam["volume"][0]
    full = _trace(ds, b, record=True)
    assert (full.prim[:1000] >= 0).any() and (full.prim[:1000] < 0).any()
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        for start in (0, 5):
            sl = slice(start, start + n)
            r = ds.trace(b.o[sl], b.d[sl], b.tm[sl], tmin=b.tmin, record=True)
            for x, y in zip(r, full):
                assert _same(x, y[sl]), (name, n, start)


@pytest.mark.parametrize("name", ["quads", "cornell_smoke", "final", "bouncing", "two_spheres"])
def test_nonfinite_ray_is_a_miss(gpu, scenes, name):
    """A ray with NaN or +-inf in any origin, direction or time component is a miss -- closest (t = FLT_MAX, prim = inst = -1),
    any hit (0) and record mode (zero records, mat -1) -- under every option, and the other rays of the batch are
    unaffected.  A zero direction is a miss as well (no special case: every hit function rejects it on its own)."""
    hs, ds, os_, fam = scenes(name)
    src = fam["volume"][0]
    nf = fam["nonfinite"][0]
    k = min(len(src.o), 3000)
    o = np.concatenate([src.o[:k], nf.o]); d = np.concatenate([src.d[:k], nf.d]); tm = np.concatenate([src.tm[:k], nf.tm])
    perm = np.random.default_rng(3).permutation(len(o))
    o, d, tm = o[perm], d[perm], tm[perm]
    bad = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1) & np.isfinite(tm)) | (d == 0).all(1)
    assert bad.sum() == len(nf.o)
    ref = ds.trace(o[~bad], d[~bad], tm[~bad], record=True)
    try:
        for lds, tree in OPTIONS:
            gpu.set_option("trace_lds", lds)
            gpu.set_option("trace_tree", tree)
            r = ds.trace(o, d, tm, record=True)
            c = ds.trace(o, d, tm)
            h = ds.trace(o, d, tm, any_hit=True)
            assert (r.t[bad] == tf.FLT_MAX).all() and (r.prim[bad] == -1).all() and (r.inst[bad] == -1).all(), (lds, tree)
            assert (r.mat[bad] == -1).all() and (r.point[bad] == 0).all() and (r.normal[bad] == 0).all() and (r.uv[bad] == 0).all()
            assert (c.t[bad] == tf.FLT_MAX).all() and (c.prim[bad] == -1).all()
            assert not h[bad].any(), (lds, tree, np.flatnonzero(h & bad)[:5])
            for x, y in zip(r, ref):
                assert _same(x[~bad], y), (lds, tree)
            assert np.array_equal(h[~bad], ref.prim >= 0)
    finally:
        gpu.reset_options()
