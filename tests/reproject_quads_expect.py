"""What rt_reproject_quads must return: a NumPy restatement of the whole extended contract in include/rt_abi.h ("temporal
reprojection that follows moved quads and boxes"): step 1 with the quad tail 1a''-1c'' in front of rt_reproject_instances' 1a'-1c'
and rt_reproject_moving's 1a-1c, step 2, step 3 with the carried normal and both id tests, step 4.

As in tests/reproject_instances_expect.py, whose helpers, record layouts and instance rule are used here, everything but the
matrix is float32 with one rounding per written operation, min and max are fmin and fmax, and the four taps are visited in the
contract's order.  Ids and inst are required; the prim and the inst test of a tap are always on.

Also here, shared by the host and the GPU tests: synthetic_quads(), the seeded buffers of the parity test with ids, inst planes and
tables that reach every branch of the three tails.
"""
from __future__ import annotations

import numpy as np

import reproject_expect as rx
import reproject_instances_expect as ix
import reproject_moving_expect as mx

F = np.float32
DEFAULTS = rx.DEFAULTS
QUAD_DTYPE = np.dtype([("Q", "<f4", 3), ("D", "<f4"), ("u", "<f4", 3), ("mat", "<i4"), ("v", "<f4", 3), ("pad0", "<f4"),
                       ("w", "<f4", 3), ("pad1", "<f4"), ("n", "<f4", 3), ("pad2", "<f4")])
INSTANCE_DTYPE = ix.INSTANCE_DTYPE
ROTATE_Y, TRANSLATE = ix.ROTATE_Y, ix.TRANSLATE
SPHERE, QUAD, BOX, INSTANCE, MEDIUM = mx.SPHERE, mx.QUAD, mx.BOX, mx.INSTANCE, mx.MEDIUM
ref = mx.ref


def _mul(a, b):
    return (a * b).astype(F)


def dot(a, b):
    """The header's dot: (a.x b.x + a.y b.y) + a.z b.z."""
    return ((_mul(a[..., 0], b[..., 0]) + _mul(a[..., 1], b[..., 1])).astype(F) + _mul(a[..., 2], b[..., 2])).astype(F)


def cross(x, y):
    """The header's cross: (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0)."""
    return np.stack([(_mul(x[..., 1], y[..., 2]) - _mul(x[..., 2], y[..., 1])).astype(F),
                     (_mul(x[..., 2], y[..., 0]) - _mul(x[..., 0], y[..., 2])).astype(F),
                     (_mul(x[..., 0], y[..., 1]) - _mul(x[..., 1], y[..., 0])).astype(F)], axis=-1)


def followed_quad(prim, inst, n_quads, n_instances):
    """Step 1a'': the quad index each pixel follows, or -1 (none: rt_reproject_instances' step 1 applies unchanged)."""
    r, ii = prim.astype(np.int64), inst.astype(np.int64)
    kind, index = (r & 0xFFFFFFFF) >> 28, r & 0x0FFFFFFF
    takes = (r >= 0) & (kind == QUAD) & (index < n_quads) & ((ii < 0) | (ii < n_instances))
    return np.where(takes, index, -1)


def quad_records_differ(G, H):
    """Step 1b'': any component of Q, u or v compares != (a NaN compares as moved); D, w, n, mat and the pads do not enter."""
    with np.errstate(all="ignore"):
        return (G["Q"] != H["Q"]).any(axis=-1) | (G["u"] != H["u"]).any(axis=-1) | (G["v"] != H["v"]).any(axis=-1)


def planar(B, G):
    """(alpha, beta) of the object-space point B in the current record's frame: quad::hit's planar coordinates, not clamped."""
    with np.errstate(all="ignore"):
        h = (B - G["Q"]).astype(F)
        return dot(G["w"], cross(h, G["v"])), dot(G["w"], cross(G["u"], h))


def carry_point(B, G, H):
    """Step 1c'' in object space: B (..., 3) float32 on the current record G -> B' on the previous record H."""
    with np.errstate(all="ignore"):
        a, b = planar(B, G)
        return np.stack([((H["Q"][..., c] + _mul(a, H["u"][..., c])).astype(F) + _mul(b, H["v"][..., c])).astype(F) for c in range(3)], axis=-1)


def carry_normal(Nb, G, H):
    """Step 1c'' for the object-space normal: the previous record's n, on the side and with the length the pixel saw."""
    with np.errstate(all="ignore"):
        s = dot(Nb, G["n"])
        return np.stack([_mul(s, H["n"][..., c]) for c in range(3)], axis=-1)


def to_object(P, I):
    """A and B of step 1c': world -> object by the current instance record."""
    with np.errstate(all="ignore"):
        A = np.where(((I["flags"] & TRANSLATE) != 0)[..., None], (P - I["offset"]).astype(F), P).astype(F)
        return rotate_in(A, I)


def rotate_in(v, I):
    with np.errstate(all="ignore"):
        rot = (I["flags"] & ROTATE_Y) != 0
        bx = np.where(rot, (_mul(I["cos_t"], v[..., 0]) - _mul(I["sin_t"], v[..., 2])).astype(F), v[..., 0])
        bz = np.where(rot, (_mul(I["sin_t"], v[..., 0]) + _mul(I["cos_t"], v[..., 2])).astype(F), v[..., 2])
        return np.stack([bx, v[..., 1], bz], axis=-1).astype(F)


def rotate_out(v, J):
    with np.errstate(all="ignore"):
        rot = (J["flags"] & ROTATE_Y) != 0
        cx = np.where(rot, (_mul(J["cos_t"], v[..., 0]) + _mul(J["sin_t"], v[..., 2])).astype(F), v[..., 0])
        cz = np.where(rot, (_mul(J["cos_t"], v[..., 2]) - _mul(J["sin_t"], v[..., 0])).astype(F), v[..., 2])
        return np.stack([cx, v[..., 1], cz], axis=-1).astype(F)


def to_world(B, J):
    """C and P' of step 1c': object -> previous world by the previous instance record."""
    with np.errstate(all="ignore"):
        C = rotate_out(B, J)
        return np.where(((J["flags"] & TRANSLATE) != 0)[..., None], (C + J["offset"]).astype(F), C).astype(F)


def reproject(color, depth, alpha, cur, prev, normal=None, prim=None, history=None, history_len=None, prev_depth=None,
              prev_alpha=None, prev_normal=None, prev_prim=None, spheres=None, prev_spheres=None, media=None, time=None, prev_time=None,
              inst=None, prev_inst=None, instances=None, prev_instances=None, quads=None, prev_quads=None,
              alpha_min=DEFAULTS["alpha_min"], depth_tol=DEFAULTS["depth_tol"], normal_min=DEFAULTS["normal_min"],
              max_history=DEFAULTS["max_history"], details=None):
    """-> (out (ny, nx, 3), out_len (ny, nx), motion (ny, nx, 2)), all float32.  quads / prev_quads: QUAD_DTYPE arrays of one
    length (None: n_quads = 0); the other tables as in reproject_instances_expect.reproject.  details: a dict that receives that
    function's entries and "quad" (step 1a''), "on_quad" (surface pixels on the quad path), "followed_quad" (those that took step
    1c'') and "under_instance" (quad-path pixels with an instance in range)."""
    assert prim is not None and prev_prim is not None and inst is not None, "ids and inst are required"
    assert (prev_inst is None) == (history is None)
    ny, nx = depth.shape
    alpha_min, depth_tol, normal_min, max_history = F(alpha_min), F(depth_tol), F(normal_min), F(max_history)
    time = mx.shutter_centre(cur) if time is None else F(time)
    prev_time = mx.shutter_centre(prev) if prev_time is None else F(prev_time)
    n_spheres = 0 if spheres is None else len(spheres)
    assert n_spheres == (0 if prev_spheres is None else len(prev_spheres))
    n_instances = 0 if instances is None else len(instances)
    assert n_instances == (0 if prev_instances is None else len(prev_instances))
    n_quads = 0 if quads is None else len(quads)
    assert n_quads == (0 if prev_quads is None else len(prev_quads))
    M = rx.matrix(prev)
    assert M is not None, "the contract refuses this previous camera"
    normals_on = history is not None and normal is not None and prev_normal is not None
    O, LL, H, V, Op = (np.array(list(v), F) for v in (cur.origin, cur.lower_left_corner, cur.horizontal, cur.vertical, prev.origin))
    with np.errstate(all="ignore"):
        fi = np.broadcast_to(np.arange(nx).astype(F)[None, :], (ny, nx))
        fj = np.broadcast_to(np.arange(ny).astype(F)[:, None], (ny, nx))
        s = ((fi + F(0.5)) / F(nx)).astype(F)
        t = ((fj + F(0.5)) / F(ny)).astype(F)
        # 1. the centre ray and the world point
        dirv = np.stack([(((LL[c] + s * H[c]).astype(F) + t * V[c]).astype(F) - O[c]).astype(F) for c in range(3)], axis=-1)
        surface = alpha >= alpha_min
        z = (depth / alpha).astype(F)
        P = np.stack([(O[c] + (z * dirv[..., c]).astype(F)).astype(F) for c in range(3)], axis=-1)
        from_prev = lambda X: np.stack([(X[..., c] - Op[c]).astype(F) for c in range(3)], axis=-1)   # noqa: E731
        qs = from_prev(P)
        # 1a' - 1c'. surface pixels on an instance whose record changed are carried back, their normals with them; a quad-path
        # pixel under an instance has that instance here too (its prim is no medium), so `imoved only` is this rule as it stands
        i = ix.followed_instance(inst, prim, n_instances, media)
        on_instance = surface & (i >= 0)
        followed = np.zeros((ny, nx), bool)
        nrm = normal
        none_i = np.zeros(1, INSTANCE_DTYPE)
        ii = np.where(i >= 0, i, 0)
        I, J = (instances[ii], prev_instances[ii]) if n_instances else (none_i[ii], none_i[ii])
        if n_instances:
            followed = on_instance & ix.records_differ(I, J)
            qs = np.where(followed[..., None], from_prev(ix.carry_point(P, I, J)), qs).astype(F)
            if normals_on:
                nrm = np.where(followed[..., None], ix.carry_normal(normal, I, J), normal).astype(F)
        # 1a'' - 1c''. surface pixels on a quad whose Q, u or v changed: in the instance's object space when there is one
        g = followed_quad(prim, inst, n_quads, n_instances)
        on_quad = surface & (g >= 0)
        followed_q = np.zeros((ny, nx), bool)
        under = on_quad & (i >= 0)
        if n_quads:
            gg = np.where(g >= 0, g, 0)
            G, Hq = quads[gg], prev_quads[gg]
            followed_q = on_quad & quad_records_differ(G, Hq)
            has_i = (i >= 0)[..., None]
            B = np.where(has_i, to_object(P, I), P).astype(F)
            Bp = carry_point(B, G, Hq)
            Pp = np.where(has_i, to_world(Bp, J), Bp).astype(F)
            qs = np.where(followed_q[..., None], from_prev(Pp), qs).astype(F)
            if normals_on:
                Nb = np.where(has_i, rotate_in(normal, I), normal).astype(F)
                Nbp = carry_normal(Nb, G, Hq)
                nrm = np.where(followed_q[..., None], np.where(has_i, rotate_out(Nbp, J), Nbp), nrm).astype(F)
        # 1a - 1c. every other surface pixel: rt_reproject_moving's sphere rule
        k = np.where(i >= 0, -1, mx.followed_sphere(prim, n_spheres, media))
        followed_sphere = np.zeros((ny, nx), bool)
        if n_spheres:
            kk = np.where(k >= 0, k, 0)
            S, T = spheres[kk], prev_spheres[kk]
            cc = np.stack([(S["c0"][..., c] + (time * S["vel"][..., c]).astype(F)).astype(F) for c in range(3)], axis=-1)
            cp = np.stack([(T["c0"][..., c] + (prev_time * T["vel"][..., c]).astype(F)).astype(F) for c in range(3)], axis=-1)
            moved = (cc != cp).any(axis=-1) | (S["radius"] != T["radius"])
            followed_sphere = surface & (k >= 0) & moved
            ratio = (T["radius"] / S["radius"]).astype(F)
            carried = np.stack([(cp[..., c] + ((P[..., c] - cc[..., c]).astype(F) * ratio).astype(F)).astype(F) for c in range(3)], axis=-1)
            qs = np.where(followed_sphere[..., None], from_prev(carried), qs).astype(F)
        if details is not None:
            details.update(instance=i, on_instance=on_instance, followed=followed, sphere=k, followed_sphere=followed_sphere,
                           quad=g, on_quad=on_quad, followed_quad=followed_q, under_instance=under)
        q = np.where(surface[..., None], qs, dirv).astype(F)
        # 2. into the previous camera
        a, b, c_ = dot(M[0], q), dot(M[1], q), dot(M[2], q)
        ahead = a > 0
        x = (((b / a).astype(F) * F(nx)).astype(F) - F(0.5)).astype(F)
        y = (((c_ / a).astype(F) * F(ny)).astype(F) - F(0.5)).astype(F)
        x0, y0 = np.floor(x).astype(F), np.floor(y).astype(F)
        fx, fy = (x - x0).astype(F), (y - y0).astype(F)
        window = ahead & (x0 >= F(-1)) & (x0 <= F(nx - 1)) & (y0 >= F(-1)) & (y0 <= F(ny - 1))
        motion = np.zeros((ny, nx, 2), F)
        motion[..., 0] = np.where(ahead, (x - fi).astype(F), F(0))
        motion[..., 1] = np.where(ahead, (y - fj).astype(F), F(0))
        out = np.array(color, F, copy=True)
        out_len = np.ones((ny, nx), F)
        if history is None:
            return out, out_len, motion
        # 3. the four taps, in order
        ix_ = np.where(window, x0, F(0)).astype(np.int64)
        iy_ = np.where(window, y0, F(0)).astype(np.int64)
        gx, gy = (F(1) - fx).astype(F), (F(1) - fy).astype(F)
        weights = [(gx * gy).astype(F), (fx * gy).astype(F), (gx * fy).astype(F), (fx * fy).astype(F)]
        W, L = np.zeros((ny, nx), F), np.zeros((ny, nx), F)
        C = np.zeros((ny, nx, 3), F)
        for tap in range(4):
            qx, qy = ix_ + (tap & 1), iy_ + (tap >> 1)
            inside = window & (qx >= 0) & (qx < nx) & (qy >= 0) & (qy < ny)
            sx, sy = np.where(inside, qx, 0), np.where(inside, qy, 0)
            hl, pa, pd = history_len[sy, sx], prev_alpha[sy, sx], prev_depth[sy, sx]
            zq = (pd / pa).astype(F)
            geo = (pa >= alpha_min) & (np.abs((zq - a).astype(F)) <= (depth_tol * np.fmax(zq, a)).astype(F))
            if normals_on:
                geo &= dot(nrm, prev_normal[sy, sx]) >= normal_min
            counts = inside & (hl > 0) & np.where(surface, geo, pa < alpha_min) & (prim == prev_prim[sy, sx]) & (inst == prev_inst[sy, sx])
            w = weights[tap]
            W = np.where(counts, (W + w).astype(F), W)
            for ch in range(3):
                C[..., ch] = np.where(counts, (C[..., ch] + (w * history[sy, sx, ch]).astype(F)).astype(F), C[..., ch])
            L = np.where(counts, (L + (w * hl).astype(F)).astype(F), L)
        # 4. blend
        have = W > 0
        n = np.fmin((L / W).astype(F), max_history).astype(F)
        length = (n + F(1)).astype(F)
        gain = (F(1) / length).astype(F)
        for ch in range(3):
            h = (C[..., ch] / W).astype(F)
            blended = (h + ((color[..., ch] - h).astype(F) * gain).astype(F)).astype(F)
            out[..., ch] = np.where(have, blended, color[..., ch])
        out_len = np.where(have, length, F(1)).astype(F)
    return out, out_len, motion


# ------------------------------------------------------------------------------------------- inputs of the parity test
def record(Q, u, v, mat=0):
    """One QUAD_DTYPE record (a 0-d array) of quad(Q, u, v): n, D and w as the constructor derives them, evaluated in double and
    rounded to float (the parity test needs records, not the host library's bits)."""
    r = np.zeros((), QUAD_DTYPE)
    Q, u, v = (np.asarray(x, np.float64) for x in (Q, u, v))
    nn = np.cross(u, v)
    with np.errstate(all="ignore"):
        unit = nn / np.sqrt(nn @ nn)
        r["Q"], r["u"], r["v"], r["mat"] = Q, u, v, mat
        r["n"], r["D"], r["w"] = unit, unit @ Q, nn / (nn @ nn)
    return r


# what each record of the quad tables is there for (index -> reason); quad_tables builds them in this order
QUAD_RECORDS = ["Q, u and v", "unmoved", "Q only", "u only", "v only", "n, w, D, mat and pads only: not moved", "nan Q", "infinite u",
                "zero w", "sheared and flipped"]
N_QUADS = len(QUAD_RECORDS)


def quad_tables():
    """(quads, prev_quads): the records of the parity test, near the points rx.synthetic's depths give."""
    cur = np.zeros(N_QUADS, QUAD_DTYPE)
    for k in range(N_QUADS):
        cur[k] = record((0.2 - 0.1 * k, -0.3 + 0.05 * k, 0.5 + 0.07 * k), (1.0 + 0.1 * k, 0.2, -0.1 * k), (0.1 * k, 0.9, 0.3 - 0.05 * k), mat=k)
    prev = cur.copy()
    prev[0] = record((0.35, -0.2, 0.4), (0.9, 0.3, 0.1), (-0.1, 1.2, 0.2), mat=0)
    prev["Q"][2] += np.array([0.05, -0.15, 0.1], F)
    prev["u"][3] += np.array([0.0, 0.25, 0.0], F)
    prev["v"][4] *= F(1.5)
    prev["n"][5], prev["w"][5], prev["D"][5], prev["mat"][5] = -cur["n"][5], cur["w"][5] * F(2), cur["D"][5] + F(1), 3
    prev["pad0"][5], prev["pad1"][5], prev["pad2"][5] = 1.0, 2.0, 3.0
    cur["Q"][6, 1] = np.nan
    prev["u"][7, 0] = np.inf
    cur["w"][8] = 0.0
    prev["Q"][8] += np.array([0.1, 0.1, 0.1], F)
    prev[9] = record(cur["Q"][9] + cur["u"][9], -cur["u"][9] + F(0.3) * cur["v"][9], cur["v"][9], mat=9)
    return cur, prev


def unmoved_quad_tables():
    """Tables of the same shape in which no record differs in Q, u or v (the NaN replaced: a NaN compares as moved); record 5 keeps
    its differences in the fields that do not enter the decision."""
    cur, prev = quad_tables()
    cur["Q"][6, 1] = 0.25
    same = cur.copy()
    for f in ("n", "w", "D", "mat", "pad0", "pad1", "pad2"):
        same[f][5] = prev[f][5]
    return cur, same


def id_palette():
    """ix.id_palette() and every quad of the tables, N_QUADS (the first out of range) and the largest index."""
    return np.concatenate([ix.id_palette(), np.array([ref(QUAD, k) for k in range(N_QUADS)] + [ref(QUAD, N_QUADS), ref(QUAD, 0x0FFFFFFF)], np.int32)])


def synthetic_quads(nx, ny, seed):
    """rx.synthetic's buffers with prim / prev_prim painted in 3 x 2 patches from id_palette() and inst / prev_inst in 4 x 3 patches
    from ix.inst_palette() -- the same patches in both frames, with one pixel in eight of each previous plane repainted at random,
    so that taps pass and fail both id tests -- and the tables of mx.tables(), ix.instance_tables() and quad_tables().  Half the
    prim patches show a quad of the tables; about a third of the frame shows no instance, a fifth the moved instance 0 and a fifth
    the unmoved instance 1, so that a moved quad meets each of them."""
    s = rx.synthetic(nx, ny, seed)
    rng = np.random.default_rng(seed + 3000)
    jj, ii = np.mgrid[0:ny, 0:nx]

    def paint(pal, weights, w, h):
        patch = (ii // w) + ((nx + w - 1) // w) * (jj // h)
        choice = rng.choice(len(pal), int(patch.max()) + 1, p=weights / weights.sum())
        if len(choice) >= len(pal):                      # every value at least once, wherever the frame has room for that
            choice[rng.permutation(len(choice))[:len(pal)]] = np.arange(len(pal))
        plane = pal[choice[patch]].astype(np.int32)
        before = plane.copy()
        again = rng.random((ny, nx)) < 0.125
        before[again] = pal[rng.integers(0, len(pal), int(again.sum()))]
        return plane, before

    pal = id_palette()
    weights = np.ones(len(pal))
    in_tables = (pal >= 0) & ((pal >> 28) == QUAD) & ((pal & 0x0FFFFFFF) < N_QUADS)
    weights[in_tables] = (len(pal) - in_tables.sum()) / in_tables.sum()
    prim, prev_prim = paint(pal, weights, 3, 2)
    ipal = ix.inst_palette()
    weights = np.ones(len(ipal))
    rest = len(ipal) - 3
    weights[0], weights[1], weights[2] = 1.25 * rest, 0.75 * rest, 0.75 * rest
    inst, prev_inst = paint(ipal, weights, 4, 3)
    b = dict(s["buffers"], prim=prim, prev_prim=prev_prim, inst=inst, prev_inst=prev_inst)
    spheres, prev_spheres, _, time, prev_time = mx.tables()
    instances, prev_instances, media = ix.instance_tables()
    quads, prev_quads = quad_tables()
    return {"cur": s["cur"], "cams": s["cams"], "buffers": b,
            "tables": dict(spheres=spheres, prev_spheres=prev_spheres, media=media, time=time, prev_time=prev_time, instances=instances,
                           prev_instances=prev_instances, quads=quads, prev_quads=prev_quads)}


select = ix.select


def without_quads(kw):
    """The same keyword arguments for reproject_instances_expect.reproject / rt_reproject_instances."""
    return {k: v for k, v in kw.items() if k not in ("quads", "prev_quads")}


# ------------------------------------------------------------------------------------ the real pairs of the GPU tests
def shows_moved(prim, inst, n_quads, n_instances, moved_indices):
    """Pixels whose step 1a'' quad is one of `moved_indices`."""
    return np.isin(followed_quad(prim, inst, n_quads, n_instances), np.asarray(moved_indices))


def box_extent(faces):
    """(a, b): per-axis min / max over the corners Q, Q + u, Q + v, (Q + u) + v of a box's six records, in float32."""
    corners = np.concatenate([faces["Q"], (faces["Q"] + faces["u"]).astype(F), (faces["Q"] + faces["v"]).astype(F),
                              ((faces["Q"] + faces["u"]).astype(F) + faces["v"]).astype(F)])
    return corners.min(axis=0), corners.max(axis=0)
