"""Ray families for the trace tests, and a plain float64 brute force over a solid scene's primitives.

Shared by tests/test_trace_oracle.py (CPU: the oracle's trace entry point) and tests/test_trace_edges.py (GPU:
rt_trace_rays against it).  Everything is deterministic: each family is drawn from a generator seeded by the scene name.

A family is a list of batches; a batch is the arguments of one trace call -- origins, directions, times, a scalar tmin and
a per-ray tmax (None = FLT_MAX) -- plus `exact`, which marks the rays built where the float64 check may say "undecided" (see
f64_check): aimed exactly at a feature (a quad edge, a sphere silhouette), or starting so far out (1e12 x the scene) that
binary32 cannot place the scene relative to the origin at all (|o - c| rounds by more than the scene's size).
"""
import collections
import ctypes as C

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
U = 2.0 ** -24                                  # unit roundoff of binary32
Batch = collections.namedtuple("Batch", "o d tm tmin tmax exact")
FINITE_FAMILIES = ["render", "volume", "aimed", "axis", "scale", "window"]
PRIM_SPHERE, PRIM_QUAD, PRIM_BOX, PRIM_INSTANCE, PRIM_MEDIUM = range(5)
INST_ROTATE_Y, INST_TRANSLATE = 1, 2


def ray_sample(orc, oscene, nx, ny, ns):
    """Every ray of an oracle render (orc_ray_sample, stride 1): (m, 8) origin, direction, time, closest t or FLT_MAX."""
    L = orc.lib()
    L.orc_ray_sample.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_void_p, C.c_int]
    cap = nx * ny * ns * 50          # at most 50 rays per sample (main.cu:54)
    rays = np.zeros((cap, 8), np.float32)
    m = L.orc_ray_sample(oscene.h, nx, ny, ns, 0, ny, 1, rays.ctypes.data, cap)
    return rays[:m].copy()


def _f32(x):
    return np.ascontiguousarray(x, np.float32)


def _batch(o, d, tm, tmin=0.001, tmax=None, exact=None):
    n = len(o)
    return Batch(_f32(o).reshape(n, 3), _f32(d).reshape(n, 3), _f32(tm).reshape(n), float(np.float32(tmin)),
                 None if tmax is None else _f32(tmax).reshape(n), np.zeros(n, bool) if exact is None else np.asarray(exact, bool))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def boxes(hs):
    if hs.desc.n_boxes == 0:
        return np.zeros(0, np.int32)
    buf = (C.c_char * (4 * hs.desc.n_boxes)).from_address(hs.desc.boxes)
    return np.frombuffer(buf, np.int32, hs.desc.n_boxes).copy()


def surfaces(hs):
    """The scene's leaf objects resolved to spheres and quads: a list of (kind, index, instance or -1) in node order, each
    with the RT_PRIM_REF rt_trace_rays reports for it (a box face is its quad).  Media are not resolved (their sample is
    a hashed draw): the float64 check is for scenes with desc.n_media == 0."""
    nodes, inst, bx = hs.nodes(), hs.instances(), boxes(hs)
    out = []

    def add(ref, k):
        kind, idx = (int(ref) & 0xFFFFFFFF) >> 28, int(ref) & 0x0FFFFFFF
        if kind == PRIM_SPHERE or kind == PRIM_QUAD:
            out.append((kind, idx, k))
        elif kind == PRIM_BOX:
            first = int(bx[idx]) & 0x3FFFFFFF
            out.extend((PRIM_QUAD, first + f, k) for f in range(6))
        elif kind == PRIM_INSTANCE:
            add(inst[idx]["child"], idx)
        else:
            raise ValueError("media are outside the float64 check")
    for ref in nodes["prim"][nodes["prim"] >= 0]:
        add(ref, -1)
    return out


def to_world(inst_rec, p):
    """Object space -> world space of translate(rotate_y(.)) in float64 (the inverse of the product's to_object_space)."""
    p = np.array(p, np.float64)
    if inst_rec["flags"] & INST_ROTATE_Y:
        c, s = float(inst_rec["cos_t"]), float(inst_rec["sin_t"])
        x, z = p[..., 0].copy(), p[..., 2].copy()
        p[..., 0], p[..., 2] = c * x + s * z, -s * x + c * z
    if inst_rec["flags"] & INST_TRANSLATE:
        p = p + inst_rec["offset"].astype(np.float64)
    return p


# ----------------------------------------------------------------------------------------------------------- ray families
def families(hs, rays, oracle_trace, n=12000, seed_name=""):
    """All families for one scene.  `rays`: ray_sample() of the scene; `oracle_trace(batch)` -> the oracle's t for a batch
    (the window family puts tmax on it).  Returns {family: [Batch, ...]} including "nonfinite"."""
    rng = np.random.default_rng([ord(c) for c in (seed_name or hs.name)])
    nodes = hs.nodes()
    lo, hi = nodes[0]["bmin"].astype(np.float64), nodes[0]["bmax"].astype(np.float64)
    ctr, half = (lo + hi) / 2, (hi - lo) / 2
    fam = {}

    # render: the oracle render's own rays with random windows (as test_trace_rays._windows)
    o, d, tm = rays[:, 0:3], rays[:, 3:6], rays[:, 6]
    t = rays[:, 7]
    base = np.where(t < FLT_MAX, t, np.float32(50.0))
    fam["render"] = [_batch(o, d, tm)] + [_batch(o, d, tm, tmin, base * rng.uniform(0.0, 1.5, len(t)) + tmin)
                                           for tmin in (0.001, 0.37, -2.0)]

    # volume: origins uniform in 1.5 x B, directions uniform on the sphere with magnitude 1e-3..1e3, times in [-0.5, 1.5]
    o = ctr + 1.5 * half * rng.uniform(-1, 1, (n, 3))
    d = _unit(rng, n) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    fam["volume"] = [_batch(o, d, rng.uniform(-0.5, 1.5, n))]

    # aimed: from inside and outside B at quad corners / edge midpoints, sphere silhouettes and node box corners
    targets, exact = [], []
    q, sph, inst = hs.quads(), (hs.spheres() if hs.desc.n_spheres else None), hs.instances()
    surf = surfaces(hs) if hs.desc.n_media == 0 else _surfaces_no_media(hs)
    k_q = [(i, k) for kind, i, k in surf if kind == PRIM_QUAD]
    k_s = [(i, k) for kind, i, k in surf if kind == PRIM_SPHERE]
    m = n // 3
    origins = np.where(rng.uniform(size=(m * 3, 1)) < 0.5, ctr + half * rng.uniform(-1, 1, (m * 3, 3)),
                       ctr + 3 * half * rng.uniform(-1, 1, (m * 3, 3)))
    tms = rng.uniform(0, 1, m * 3)
    if k_q:
        pick = rng.integers(0, len(k_q), m)
        w = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [.5, 0], [0, .5], [1, .5], [.5, 1]])[rng.integers(0, 8, m)]
        for j in range(m):
            i, k = k_q[pick[j]]
            p = q[i]["Q"].astype(np.float64) + w[j, 0] * q[i]["u"] + w[j, 1] * q[i]["v"]
            targets.append(p if k < 0 else to_world(inst[k], p))
    if k_s:
        pick = rng.integers(0, len(k_s), m)
        for j in range(m):
            i, k = k_s[pick[j]]
            s = sph[i]
            c = s["c0"].astype(np.float64) + np.float64(np.float32(tms[len(targets)])) * s["vel"]
            cw = c if k < 0 else to_world(inst[k], c)
            a = cw - origins[len(targets)]
            perp = np.cross(a, rng.normal(size=3))
            perp /= np.linalg.norm(perp)
            p_obj = c + abs(float(s["radius"])) * (perp if k < 0 else _rot_to_obj(inst[k], perp))
            targets.append(p_obj if k < 0 else to_world(inst[k], p_obj))
    n_exact = len(targets)
    corners = rng.integers(0, 2, (m, 3))
    ni = rng.integers(0, len(nodes), m)
    for j in range(m):
        targets.append(np.where(corners[j] == 1, nodes[ni[j]]["bmax"], nodes[ni[j]]["bmin"]).astype(np.float64))
    targets = np.array(targets)
    nt = len(targets)
    exact = np.arange(nt) < n_exact
    # half aimed exactly, half nudged by 1e-4 of the scene size (those are not on the feature)
    nudge = np.where(rng.uniform(size=(nt, 1)) < 0.5, 0.0, 1e-4 * np.abs(half).max() * _unit(rng, nt))
    exact &= nudge[:, 0] == 0
    tgt = _f32(targets + nudge)
    ob = _f32(origins[:nt])
    fam["aimed"] = [_batch(ob, tgt - ob, tms[:nt], exact=exact)]

    # axis: one or two direction components exactly +-0, origin coordinates copied from node bounds
    o = ctr + half * rng.uniform(-1, 1, (n, 3))
    ni = rng.integers(0, len(nodes), (n, 3))
    bnd = np.where(rng.uniform(size=(n, 3)) < 0.5, nodes["bmin"][ni, np.arange(3)], nodes["bmax"][ni, np.arange(3)])
    copy = rng.uniform(size=(n, 3)) < 0.5
    o = np.where(copy, bnd, o)
    d = _f32(_unit(rng, n))
    nz = rng.integers(1, 3, n)
    for j in range(n):
        ax = rng.permutation(3)[:nz[j]]
        d[j, ax] = np.where(rng.uniform(size=len(ax)) < 0.5, np.float32(0.0), np.float32(-0.0))
    fam["axis"] = [_batch(o, d, rng.uniform(0, 1, n))]

    # scale: tiny direction components, huge direction magnitudes, far origins aimed at B
    m = n // 3
    o = ctr + half * rng.uniform(-1, 1, (m, 3))
    d = _f32(_unit(rng, m) * 10.0 ** rng.uniform(-1, 1, (m, 1)))
    tiny = np.array([1e-20, 1e-27, 1e-30, 1e-38, 1e-40, 1e-45], np.float32)
    d[np.arange(m), rng.integers(0, 3, m)] = tiny[rng.integers(0, len(tiny), m)] * np.where(rng.uniform(size=m) < .5, 1, -1)
    b_tiny = _batch(o, d, rng.uniform(0, 1, m))
    o = ctr + half * rng.uniform(-1, 1, (m, 3))
    b_big = _batch(o, _unit(rng, m) * 10.0 ** rng.uniform(3, 19, (m, 1)), rng.uniform(0, 1, m))
    far = np.array([1e3, 1e6, 1e12])[rng.integers(0, 3, m)][:, None] * np.abs(half).max()
    o = ctr + far * _unit(rng, m)
    tgt = ctr + 0.3 * half * rng.uniform(-1, 1, (m, 3))
    fam["scale"] = [b_tiny, b_big, _batch(o, (tgt - o) / np.linalg.norm(tgt - o, axis=1, keepdims=True), rng.uniform(0, 1, m),
                                          exact=far[:, 0] > 1e9 * np.abs(half).max())]

    # window edges: tmax at the oracle's t and one ulp either side; +inf, -inf, 0, tmin, below tmin; scalar tmin sweep
    src = fam["volume"][0]
    sel = slice(0, min(n, 4000))
    o, d, tm = src.o[sel], src.d[sel], src.tm[sel]
    t = oracle_trace(_batch(o, d, tm))
    hit = t < FLT_MAX
    o, d, tm, t = o[hit], d[hit], tm[hit], t[hit]
    w = [_batch(o, d, tm, 0.001, t), _batch(o, d, tm, 0.001, np.nextafter(t, np.float32(np.inf))),
         _batch(o, d, tm, 0.001, np.nextafter(t, np.float32(-np.inf)))]
    nn = len(src.o[sel])
    o, d, tm = src.o[sel], src.d[sel], src.tm[sel]
    for v in (np.inf, -np.inf, 0.0, 0.001, -1.0):
        w.append(_batch(o, d, tm, 0.001, np.full(nn, v, np.float32)))
    for tmin in (0.0, 1e-30, 0.001, 1.0, 100.0, -1e30):
        w.append(_batch(o, d, tm, tmin))
    fam["window"] = w

    # non-finite: NaN / +-inf in each origin, direction and time component of otherwise ordinary rays; a zero direction
    base = fam["volume"][0]
    k = min(n, 2000)
    o, d, tm = [], [], []
    for slot in range(7):
        for v in (np.nan, np.inf, -np.inf):
            oo, dd, tt = base.o[:k].copy(), base.d[:k].copy(), base.tm[:k].copy()
            if slot < 3:
                oo[:, slot] = v
            elif slot < 6:
                dd[:, slot - 3] = v
            else:
                tt[:] = v
            o.append(oo), d.append(dd), tm.append(tt)
    o.append(base.o[:k]), d.append(np.zeros((k, 3), np.float32)), tm.append(base.tm[:k])
    fam["nonfinite"] = [_batch(np.concatenate(o), np.concatenate(d), np.concatenate(tm))]
    return fam


def _rot_to_obj(inst_rec, v):
    """A world-space direction into object space (the rotation only)."""
    v = np.array(v, np.float64)
    if inst_rec["flags"] & INST_ROTATE_Y:
        c, s = float(inst_rec["cos_t"]), float(inst_rec["sin_t"])
        return np.array([c * v[0] - s * v[2], v[1], s * v[0] + c * v[2]])
    return v


def _surfaces_no_media(hs):
    """surfaces() with media left out (for aiming only: a medium's boundary is one of the other leaves' kind)."""
    nodes, inst, bx = hs.nodes(), hs.instances(), boxes(hs)
    media = hs.media()
    out = []

    def add(ref, k):
        kind, idx = (int(ref) & 0xFFFFFFFF) >> 28, int(ref) & 0x0FFFFFFF
        if kind in (PRIM_SPHERE, PRIM_QUAD):
            out.append((kind, idx, k))
        elif kind == PRIM_BOX:
            out.extend((PRIM_QUAD, (int(bx[idx]) & 0x3FFFFFFF) + f, k) for f in range(6))
        elif kind == PRIM_INSTANCE:
            add(inst[idx]["child"], idx)
        elif kind == PRIM_MEDIUM:
            add(media[idx]["boundary"], k)
    for ref in nodes["prim"][nodes["prim"] >= 0]:
        add(ref, -1)
    return out


def expected_nonfinite_miss(b):
    """The product's rule: a ray with a non-finite origin, direction or time is a miss."""
    return ~(np.isfinite(b.o).all(1) & np.isfinite(b.d).all(1) & np.isfinite(b.tm))


# -------------------------------------------------------------------------------------------------------- float64 check
F64Result = collections.namedtuple("F64Result", "off_surface missed undecided overflow")


def f64_check(hs, b, t, prim, inst, chunk=256):
    """Checks a closest-hit answer (t, prim, inst per ray; prim -2 on a hit = some primitive, for the oracle, which reports none) for batch `b` against a float64 brute force over every sphere and
    quad of a solid scene (no BVH; instances through their transform evaluated in float64 from the stored sin, cos and
    offset).  Returns the indices of rays that fail each check and of rays whose check was weakened:

    * off_surface: a reported hit whose primitive, evaluated in float64 along the same object-space ray, has no root within
      E of t;
    * missed: some primitive has a float64 hit inside the window that is clearly before the reported t (by more than the
      two bounds together), or a reported miss while some primitive has a clear hit in the window;
    * undecided: rays for which a candidate that could have changed the answer was ambiguous -- a sphere discriminant
      within its error of 0 (grazing), alpha or beta within their error of 0 or 1 (an edge), |n.d| within its error of the
      reference's 1e-8 cut, and a quad whose t lies within its error of the window's ends (those are decided bit for bit
      against the oracle, not here);
    * overflow: rays for which a binary32 intermediate of some candidate overflows (|b|^2, a c or a beyond FLT_MAX / 4 for a
      sphere; |t d| for a quad): the reference's float arithmetic then answers differently from real arithmetic by
      design, and the bound below does not apply.

    The bounds (u = 2^-24, every binary32 operation rounds with relative error <= u, and a dot product of three terms with
    two fmas is within 3u of the sum of its terms' magnitudes):

    * transform: o' = R (o - off) is within 4u (|o| + |off|) of exact per component, d' = R d within 3u |d|;
    * sphere: with oc = o' - c(tm) (o is the caller's float, exact; c(tm) is one fma, within 2u (|c0| + |tm vel|); the
      subtraction rounds once), E_oc = 2u (|c0| + |tm vel|) + u |oc| + the transform's error.  Then E_b = |d| E_oc + 3u |oc| |d| + |oc| 3u |d| (b = oc.d), E_a = 3u a + 6u a,
      E_c = 2 |oc| E_oc + 3u (|oc|^2 + r^2), E_disc = 2 |b| E_b + a E_c + |c| E_a + 3u (b^2 + a |c|), E_sq = E_disc /
      (2 sq) (sq = sqrt(disc) > 0), and t = (-b -+ sq) / a within E = (E_b + E_sq + 2u (|b| + sq)) / a + |t| (E_a / a +
      u).  The discriminant is undecided where |disc| <= E_disc.
    * quad: denom = n.d' within E_den = 3u sum |n_i| |d'_i| + |n| 3u |d|, num = D - n.o' within E_num = 4u (|D| +
      sum |n_i| |o'_i|) + |n| 4u (|o| + |off|); t = num / denom within E = (E_num + |t| E_den) / |denom| + u |t|.  alpha
      = w . ((P - Q) x v) with P = o' + t d' (within E_P = E |d'| + 2u (|o'| + |t d'|) + the transform's error) is within
      E_alpha = |w| |v| (E_P + 4u (|P| + |Q|)) + 6u |w| |v| |P - Q|, beta likewise with |u|.

    Every bound is then doubled: the terms above are first order, and the doubling covers the second-order ones (all of
    order u^2 relative, since no intermediate overflows or underflows outside the rays counted as overflow)."""
    sph = hs.spheres() if hs.desc.n_spheres else None
    q, insts = hs.quads(), hs.instances()
    surf = surfaces(hs)
    n = len(b.o)
    tmax = np.full(n, FLT_MAX, np.float64) if b.tmax is None else b.tmax.astype(np.float64)
    tmin = float(b.tmin)
    t = np.asarray(t).astype(np.float64)
    prim, inst = np.asarray(prim).astype(np.int64), np.asarray(inst).astype(np.int64)
    hit = prim != -1
    off_surface, missed = [], []
    undecided, overflow = [], []

    groups = {}
    for kind, idx, k in surf:
        groups.setdefault(k, ([], []))[0 if kind == PRIM_SPHERE else 1].append(idx)
    for c0 in range(0, n, chunk):
        sl = slice(c0, min(n, c0 + chunk))
        o, d, tm = b.o[sl].astype(np.float64), b.d[sl].astype(np.float64), b.tm[sl].astype(np.float64)
        lo_w, hi_w = tmin, tmax[sl]
        r = len(o)
        best = np.full(r, np.inf)        # earliest clear hit of any candidate
        best_e = np.zeros(r)
        rep_ok = ~hit[sl]                # reported hit found on its surface
        rep_e = np.zeros(r)              # the bound of the reported hit's root
        undec = np.zeros(r, bool)        # an ambiguous candidate before the reported t
        ovf = np.zeros(r, bool)
        t_rep = np.where(hit[sl], t[sl], np.inf)
        for k, (s_idx, q_idx) in groups.items():
            if k >= 0:
                ir = insts[k]
                off = ir["offset"].astype(np.float64) if ir["flags"] & INST_TRANSLATE else np.zeros(3)
                oo, dd = o - off, d.copy()
                if ir["flags"] & INST_ROTATE_Y:
                    cs, sn = float(ir["cos_t"]), float(ir["sin_t"])
                    oo = np.stack([cs * oo[:, 0] - sn * oo[:, 2], oo[:, 1], sn * oo[:, 0] + cs * oo[:, 2]], 1)
                    dd = np.stack([cs * dd[:, 0] - sn * dd[:, 2], dd[:, 1], sn * dd[:, 0] + cs * dd[:, 2]], 1)
                e_tr = 4 * U * (np.abs(o).sum(1) + np.abs(off).sum())      # per ray: error of o' (absolute)
                e_trd = 3 * U * np.abs(d).sum(1)                              # error of d'
            else:
                oo, dd = o, d
                e_tr = np.zeros(r)
                e_trd = np.zeros(r)
            mine = hit[sl] & ((inst[sl] == k) | (prim[sl] == -2))
            if s_idx:
                s = sph[np.array(s_idx)]
                res = _spheres64(oo, dd, tm, s, e_tr, e_trd, lo_w, hi_w)
                _merge(res, np.array([(PRIM_SPHERE << 28) | i for i in s_idx]), prim[sl], mine, t_rep,
                       best, best_e, rep_ok, rep_e, undec, ovf)
            if q_idx:
                qq = q[np.array(q_idx)]
                res = _quads64(oo, dd, qq, e_tr, e_trd, lo_w, hi_w)
                _merge(res, np.array([(PRIM_QUAD << 28) | i for i in q_idx]), prim[sl], mine, t_rep,
                       best, best_e, rep_ok, rep_e, undec, ovf)
        idx = np.arange(c0, sl.stop)
        off_surface.extend(idx[~rep_ok & ~ovf])
        # clear miss: a candidate's clear hit lies before the reported t by more than both bounds
        bad = np.isfinite(best) & (best + best_e < t_rep - rep_e) & ~ovf & ~undec
        missed.extend(idx[bad])
        undecided.extend(idx[undec & ~ovf])
        overflow.extend(idx[ovf])
    return F64Result(*(np.array(x, int) for x in (off_surface, missed, undecided, overflow)))


def _merge(res, refs, prim, mine, t_rep, best, best_e, rep_ok, rep_e, undec, ovf):
    """Fold one group's per-candidate float64 results into the per-ray state of f64_check."""
    roots, root_e, acc_t, acc_e, amb, over = res           # (r, m, 2), (r, m, 2), (r, m), (r, m), (r, m), (r, m)
    me = mine[:, None] & ((prim[:, None] == refs[None, :]) | (prim[:, None] == -2))  # the reported primitive (-2: any)
    dist = np.abs(roots - t_rep[:, None, None])
    near = (dist <= root_e).any(2)
    rep_ok |= (me & (near | over | amb)).any(1)
    e_me = np.where(me[..., None] & (dist <= root_e), root_e, 0.0).max((1, 2))
    np.maximum(rep_e, e_me, out=rep_e)
    ovf |= (over & (acc_t <= t_rep[:, None] + acc_e) | (me & over)).any(1)
    clear = np.isfinite(acc_t) & ~amb & ~over
    tt = np.where(clear, acc_t, np.inf)
    j = tt.argmin(1)
    cand = tt[np.arange(len(tt)), j]
    cand_e = acc_e[np.arange(len(tt)), j]
    take = cand < best
    best[take], best_e[take] = cand[take], cand_e[take]
    first = np.where(np.isnan(roots), np.inf, roots - root_e).min(2)
    undec |= (amb & ~over & (first <= t_rep[:, None])).any(1)


def _spheres64(o, d, tm, s, e_tr, e_trd, tmin, tmax):
    c0, vel, rad = s["c0"].astype(np.float64), s["vel"].astype(np.float64), s["radius"].astype(np.float64)
    c = c0[None] + tm[:, None, None] * vel[None]                   # (r, m, 3)
    oc = o[:, None, :] - c
    a = (d * d).sum(1)[:, None]
    bb = (oc * d[:, None, :]).sum(2)
    cc = (oc * oc).sum(2) - rad[None] ** 2
    disc = bb * bb - a * cc
    n_d = np.linalg.norm(d, axis=1)[:, None]
    n_oc = np.linalg.norm(oc, axis=2)
    e_oc = 2 * U * (np.linalg.norm(c0, axis=1)[None] + np.abs(tm)[:, None] * np.linalg.norm(vel, axis=1)[None]) + U * n_oc + e_tr[:, None]
    e_b = n_d * e_oc + 6 * U * n_oc * n_d + n_oc * e_trd[:, None]
    e_a = 9 * U * a + 2 * n_d * e_trd[:, None]
    e_c = 2 * n_oc * e_oc + 3 * U * (n_oc ** 2 + rad[None] ** 2)
    e_disc = 2 * np.abs(bb) * e_b + a * e_c + np.abs(cc) * e_a + 3 * U * (bb * bb + a * np.abs(cc))
    over = (bb * bb > FLT_MAX / 4) | (a * np.abs(cc) > FLT_MAX / 4) | (a > FLT_MAX / 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(np.maximum(disc, 0.0))
        e_sq = np.where(sq > 0, e_disc / (2 * sq), np.inf)
        t1, t2 = (-bb - sq) / a, (-bb + sq) / a
        roots = np.stack([t1, t2], 2)
        e = 2 * ((e_b + e_sq + 2 * U * (np.abs(bb) + sq))[..., None] / a[..., None] + np.abs(roots) * (e_a / a + U)[..., None])
    real = disc > 0
    amb = np.abs(disc) <= 2 * e_disc
    roots = np.where(real[..., None], roots, np.nan)
    # the accepted root: the first one strictly inside (tmin, tmax); a root within its bound of an end is ambiguous
    tmax_ = np.broadcast_to(np.asarray(tmax, np.float64).reshape(-1, 1, 1), roots.shape)
    inside = (roots > tmin) & (roots < tmax_)
    edge = (np.abs(roots - tmin) <= e) | (np.abs(roots - tmax_) <= e)
    first = inside[..., 0]
    acc_t = np.where(first, roots[..., 0], np.where(inside[..., 1], roots[..., 1], np.inf))
    acc_e = np.where(first, e[..., 0], e[..., 1])
    amb = amb | (real & (edge[..., 0] | (~first & edge[..., 1])))
    return roots, e, acc_t, acc_e, amb, over


def _quads64(o, d, q, e_tr, e_trd, tmin, tmax):
    n = q["n"].astype(np.float64)
    D = q["D"].astype(np.float64)
    Q, u, v, w = (q[f].astype(np.float64) for f in ("Q", "u", "v", "w"))
    denom = d @ n.T                                                  # (r, m)
    num = D[None] - o @ n.T
    e_den = 3 * U * (np.abs(d) @ np.abs(n).T) + np.linalg.norm(n, axis=1)[None] * e_trd[:, None]
    e_num = 4 * U * (np.abs(D)[None] + np.abs(o) @ np.abs(n).T) + np.linalg.norm(n, axis=1)[None] * e_tr[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = num / denom
        e_t = 2 * ((e_num + np.abs(t) * e_den) / np.abs(denom) + U * np.abs(t))
        P = o[:, None, :] + t[..., None] * d[:, None, :]
        pl = P - Q[None]
        alpha = (w[None] * np.cross(pl, v[None])).sum(2)
        beta = (w[None] * np.cross(u[None], pl)).sum(2)
        n_d = np.linalg.norm(d, axis=1)[:, None]
        n_P = np.linalg.norm(P, axis=2)
        e_P = e_t * n_d + 2 * U * (np.linalg.norm(o, axis=1)[:, None] + np.abs(t) * n_d) + e_tr[:, None] + np.abs(t) * e_trd[:, None]
        nw = np.linalg.norm(w, axis=1)[None]
        base = e_P + 4 * U * (n_P + np.linalg.norm(Q, axis=1)[None]) + 6 * U * np.linalg.norm(pl, axis=2)
        e_al = 2 * nw * np.linalg.norm(v, axis=1)[None] * base
        e_be = 2 * nw * np.linalg.norm(u, axis=1)[None] * base
    tmax_ = np.broadcast_to(np.asarray(tmax, np.float64).reshape(-1, 1), t.shape)
    over = np.isfinite(t) & (np.abs(t) * n_d > FLT_MAX / 4) & (t >= tmin) & (t <= tmax_)
    cut = np.abs(denom) >= 1e-8
    inside = cut & (t >= tmin) & (t <= tmax_) & (alpha >= 0) & (alpha <= 1) & (beta >= 0) & (beta <= 1)
    amb = (np.abs(np.abs(denom) - 1e-8) <= 2 * e_den) & (np.abs(t) < np.inf)
    on_plane = np.isfinite(t)
    amb |= on_plane & ((np.abs(alpha) <= e_al) | (np.abs(alpha - 1) <= e_al) | (np.abs(beta) <= e_be) | (np.abs(beta - 1) <= e_be))
    amb |= on_plane & ((np.abs(t - tmin) <= e_t) | (np.abs(t - tmax_) <= e_t))
    acc_t = np.where(inside, t, np.inf)
    return t[..., None].repeat(2, 2), e_t[..., None].repeat(2, 2), acc_t, e_t, amb, over
