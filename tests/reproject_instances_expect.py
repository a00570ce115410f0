"""What rt_reproject_instances must return: a NumPy restatement of the whole extended contract in include/rt_abi.h ("temporal
reprojection that follows moved instances"): step 1 with the instance tail 1a'-1c' in front of rt_reproject_moving's 1a-1c, step
2, step 3 with the carried normal and the inst test, step 4.

As in tests/reproject_moving_expect.py, whose step 1a, record layouts and helpers are used here, everything but the matrix is
float32 with one rounding per written operation, min and max are fmin and fmax, and the four taps are visited in the contract's
order.  Ids and inst are required; the prim and the inst test of a tap are always on.

Also here, shared by the host and the GPU tests: synthetic_instances(), the seeded buffers of the parity test with ids, inst planes
and tables that reach every branch of both tails.
"""
from __future__ import annotations

import numpy as np

import reproject_expect as rx
import reproject_moving_expect as mx

F = np.float32
DEFAULTS = rx.DEFAULTS
INSTANCE_DTYPE = np.dtype([("sin_t", "<f4"), ("cos_t", "<f4"), ("offset", "<f4", 3), ("child", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
ROTATE_Y, TRANSLATE = 1, 2
SPHERE, QUAD, BOX, INSTANCE, MEDIUM = mx.SPHERE, mx.QUAD, mx.BOX, mx.INSTANCE, mx.MEDIUM
ref = mx.ref


def followed_instance(inst, prim, n_instances, media):
    """Step 1a': the instance index each pixel follows, or -1 (none: steps 1a-1c of rt_reproject_moving apply)."""
    ii = inst.astype(np.int64)
    i = np.where(ii >= 0, ii, -1)
    n_media = 0 if media is None else len(media)
    if n_media:
        r = prim.astype(np.int64)
        kind, index = (r & 0xFFFFFFFF) >> 28, r & 0x0FFFFFFF
        in_medium = (ii < 0) & (r >= 0) & (kind == MEDIUM) & (index < n_media)
        b = media["boundary"][np.where(in_medium, index, 0)].astype(np.int64)
        i = np.where(in_medium & (b >= 0) & (((b & 0xFFFFFFFF) >> 28) == INSTANCE), b & 0x0FFFFFFF, i)
    return np.where((i >= 0) & (i < n_instances), i, -1)


def records_differ(I, J):
    """Step 1b': a NaN compares as moved; child and pad are not looked at."""
    with np.errstate(all="ignore"):
        return (I["sin_t"] != J["sin_t"]) | (I["cos_t"] != J["cos_t"]) | (I["offset"] != J["offset"]).any(axis=-1) | (I["flags"] != J["flags"])


def _rotations(v, I, J):
    """v (..., 3) through the current record's world -> object rotation and the previous record's object -> world rotation."""
    rot_i, rot_j = (I["flags"] & ROTATE_Y) != 0, (J["flags"] & ROTATE_Y) != 0
    bx = np.where(rot_i, ((I["cos_t"] * v[..., 0]).astype(F) - (I["sin_t"] * v[..., 2]).astype(F)).astype(F), v[..., 0])
    bz = np.where(rot_i, ((I["sin_t"] * v[..., 0]).astype(F) + (I["cos_t"] * v[..., 2]).astype(F)).astype(F), v[..., 2])
    cx = np.where(rot_j, ((J["cos_t"] * bx).astype(F) + (J["sin_t"] * bz).astype(F)).astype(F), bx)
    cz = np.where(rot_j, ((J["cos_t"] * bz).astype(F) - (J["sin_t"] * bx).astype(F)).astype(F), bz)
    return np.stack([cx, v[..., 1], cz], axis=-1).astype(F)


def carry_point(P, I, J):
    """Step 1c' up to P': P (..., 3) float32, I and J records broadcastable against P's leading shape."""
    with np.errstate(all="ignore"):
        A = np.where(((I["flags"] & TRANSLATE) != 0)[..., None], (P - I["offset"]).astype(F), P).astype(F)
        C = _rotations(A, I, J)
        return np.where(((J["flags"] & TRANSLATE) != 0)[..., None], (C + J["offset"]).astype(F), C).astype(F)


def carry_normal(N, I, J):
    with np.errstate(all="ignore"):
        return _rotations(N, I, J)


def reproject(color, depth, alpha, cur, prev, normal=None, prim=None, history=None, history_len=None, prev_depth=None,
              prev_alpha=None, prev_normal=None, prev_prim=None, spheres=None, prev_spheres=None, media=None, time=None, prev_time=None,
              inst=None, prev_inst=None, instances=None, prev_instances=None,
              alpha_min=DEFAULTS["alpha_min"], depth_tol=DEFAULTS["depth_tol"], normal_min=DEFAULTS["normal_min"],
              max_history=DEFAULTS["max_history"], details=None):
    """-> (out (ny, nx, 3), out_len (ny, nx), motion (ny, nx, 2)), all float32.  instances / prev_instances: INSTANCE_DTYPE arrays
    of one length (None: n_instances = 0); the sphere tables as in reproject_moving_expect.reproject.  details: a dict that
    receives "instance" (step 1a'), "on_instance" (surface pixels that took the instance path), "followed" (those that took step
    1c'), "sphere" (step 1a, -1 on the instance path) and "followed_sphere" (pixels that took step 1c)."""
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
    M = rx.matrix(prev)
    assert M is not None, "the contract refuses this previous camera"
    normals_on = history is not None and normal is not None and prev_normal is not None
    O, LL, H, V, Op = (np.array(list(v), F) for v in (cur.origin, cur.lower_left_corner, cur.horizontal, cur.vertical, prev.origin))
    dot = lambda a, b: ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)   # noqa: E731
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
        qs = np.stack([(P[..., c] - Op[c]).astype(F) for c in range(3)], axis=-1)
        # 1a' - 1c'. surface pixels on an instance whose record changed are carried back, their normals with them
        i = followed_instance(inst, prim, n_instances, media)
        on_instance = surface & (i >= 0)
        followed = np.zeros((ny, nx), bool)
        nrm = normal
        if n_instances:
            ii = np.where(i >= 0, i, 0)
            I, J = instances[ii], prev_instances[ii]
            followed = on_instance & records_differ(I, J)
            carried = carry_point(P, I, J)
            qm = np.stack([(carried[..., c] - Op[c]).astype(F) for c in range(3)], axis=-1)
            qs = np.where(followed[..., None], qm, qs).astype(F)
            if normals_on:
                nrm = np.where(followed[..., None], carry_normal(normal, I, J), normal).astype(F)
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
            qm = np.stack([(carried[..., c] - Op[c]).astype(F) for c in range(3)], axis=-1)
            qs = np.where(followed_sphere[..., None], qm, qs).astype(F)
        if details is not None:
            details.update(instance=i, on_instance=on_instance, followed=followed, sphere=k, followed_sphere=followed_sphere)
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
        ix = np.where(window, x0, F(0)).astype(np.int64)
        iy = np.where(window, y0, F(0)).astype(np.int64)
        gx, gy = (F(1) - fx).astype(F), (F(1) - fy).astype(F)
        weights = [(gx * gy).astype(F), (fx * gy).astype(F), (gx * fy).astype(F), (fx * fy).astype(F)]
        W, L = np.zeros((ny, nx), F), np.zeros((ny, nx), F)
        C = np.zeros((ny, nx, 3), F)
        for tap in range(4):
            qx, qy = ix + (tap & 1), iy + (tap >> 1)
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
        g = (F(1) / length).astype(F)
        for ch in range(3):
            h = (C[..., ch] / W).astype(F)
            blended = (h + ((color[..., ch] - h).astype(F) * g).astype(F)).astype(F)
            out[..., ch] = np.where(have, blended, color[..., ch])
        out_len = np.where(have, length, F(1)).astype(F)
    return out, out_len, motion


# ------------------------------------------------------------------------------------------- inputs of the parity test
def record(angle_degrees=None, offset=None, child=0):
    """One INSTANCE_DTYPE record (a 0-d array) of translate(rotate_y(child, angle), offset), either half left out when None; sin and
    cos in double, rounded to float."""
    r = np.zeros((), INSTANCE_DTYPE)
    r["cos_t"] = 1.0
    r["child"] = child
    if angle_degrees is not None:
        r["sin_t"], r["cos_t"], r["flags"] = np.sin(np.radians(angle_degrees)), np.cos(np.radians(angle_degrees)), ROTATE_Y
    if offset is not None:
        r["offset"], r["flags"] = offset, r["flags"] | TRANSLATE
    return r


# what each record of the instance tables is there for (index -> reason); instance_tables builds them in this order
INSTANCE_RECORDS = ["angle and offset", "unmoved", "offset only", "angle only", "flags only: rotate gained", "flags only: translate lost",
                    "flags 0, another offset", "flags 7", "nan sin_t", "infinite previous offset", "no sine / cosine pair", "bounds a medium"]
N_INSTANCES = len(INSTANCE_RECORDS)
N_MEDIA = 9


def instance_tables():
    """(instances, prev_instances, media): the records of the parity test, and mx.tables()' media extended by boundaries that are
    instances in and out of range."""
    cur = np.zeros(N_INSTANCES, INSTANCE_DTYPE)
    for k in range(N_INSTANCES):
        cur[k] = record(3.0 + 2.0 * k, (0.05 * k, -0.02 * k, 0.1 - 0.03 * k), child=ref(BOX, k))
    prev = cur.copy()
    prev[0] = record(-2.0, (0.12, 0.05, -0.08), child=ref(BOX, 0))
    prev["offset"][2] += np.array([0.15, -0.1, 0.05], F)
    prev[3] = record(1.5, cur["offset"][3], child=ref(BOX, 3))
    prev["flags"][4] = TRANSLATE                                     # the current frame gained the rotation
    cur["flags"][5] = ROTATE_Y                                       # ... and lost the translation
    cur["flags"][6] = prev["flags"][6] = 0                           # moved by the rule, carried by nothing
    prev["offset"][6] += np.array([0.3, 0.0, 0.0], F)
    cur["flags"][7] = prev["flags"][7] = 7                           # a bit outside 1..3 is only ever tested
    prev["sin_t"][7], prev["cos_t"][7] = np.sin(np.radians(14.0)), np.cos(np.radians(14.0))
    cur["sin_t"][8] = np.nan
    prev["offset"][9, 1] = np.inf
    cur["sin_t"][10], cur["cos_t"][10] = 0.8, 0.9
    prev["sin_t"][10], prev["cos_t"][10] = 0.5, 0.5
    prev[11] = record(20.0, (0.6, -0.1, -0.2), child=ref(SPHERE, 0))
    cur["child"][11] = ref(SPHERE, 0)
    media = np.zeros(N_MEDIA, mx.MEDIUM_DTYPE)
    media["boundary"] = list(mx.tables()[2]["boundary"]) + [ref(INSTANCE, 11), ref(INSTANCE, N_INSTANCES), ref(INSTANCE, 0x0FFFFFFF)]
    media["neg_inv_density"] = -1.0
    assert ref(INSTANCE, 0) == media["boundary"][5]
    return cur, prev, media


def unmoved_instance_tables():
    """Tables of the same shape in which no record differs (the NaN replaced: a NaN compares as moved)."""
    cur, _, media = instance_tables()
    cur["sin_t"][8] = 0.3
    return cur, cur.copy(), media


def id_palette():
    """mx.id_palette() for N_MEDIA media: media 6..8 are in range here, N_MEDIA is the first that is not."""
    return np.concatenate([mx.id_palette(), np.array([ref(MEDIUM, 7), ref(MEDIUM, 8), ref(MEDIUM, N_MEDIA)], np.int32)])


def inst_palette():
    """The values the inst planes are painted with: none (-1), every record, out of range, and negative but not -1."""
    return np.array([-1] + list(range(N_INSTANCES)) + [N_INSTANCES, 0x7FFFFFFF, -2, -2147483648], np.int32)


def synthetic_instances(nx, ny, seed):
    """rx.synthetic's buffers with prim / prev_prim painted in 3 x 2 patches from id_palette() and inst / prev_inst in 4 x 3 patches
    from inst_palette() -- the same patches in both frames, with one pixel in eight of each previous plane repainted at random,
    so that taps pass and fail both id tests -- and the tables of mx.tables() and instance_tables().  About half the frame shows
    no instance; the media come up more often than the other ids, so that every boundary rule decides pixels."""
    s = rx.synthetic(nx, ny, seed)
    rng = np.random.default_rng(seed + 2000)
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
    weights[[1, 10]] = 3.0
    weights[(pal >= 0) & ((pal >> 28) == MEDIUM)] = 3.0
    prim, prev_prim = paint(pal, weights, 3, 2)
    ipal = inst_palette()
    weights = np.ones(len(ipal))
    weights[0] = len(ipal)
    inst, prev_inst = paint(ipal, weights, 4, 3)
    b = dict(s["buffers"], prim=prim, prev_prim=prev_prim, inst=inst, prev_inst=prev_inst)
    spheres, prev_spheres, _, time, prev_time = mx.tables()
    instances, prev_instances, media = instance_tables()
    return {"cur": s["cur"], "cams": s["cams"], "buffers": b,
            "tables": dict(spheres=spheres, prev_spheres=prev_spheres, media=media, time=time, prev_time=prev_time, instances=instances,
                           prev_instances=prev_instances)}


def select(buffers, normals, history=True):
    """The keyword arguments of reproject() with the normal test on or off; ids and inst always."""
    keep = ["color", "depth", "alpha", "prim", "prev_prim", "inst"] + (["history", "history_len", "prev_depth", "prev_alpha", "prev_inst"] if history else [])
    keep += ["normal", "prev_normal"] if normals else []
    return {k: buffers[k] for k in keep}


def without_inst(kw):
    """The same keyword arguments for reproject_moving_expect.reproject / rt_reproject_moving."""
    return {k: v for k, v in kw.items() if k not in ("inst", "prev_inst", "instances", "prev_instances")}


# ------------------------------------------------------------------------------------ the real pairs of the GPU tests
def turned(records, indices, degrees, shift=(0.0, 0.0, 0.0)):
    """The records `indices` of an INSTANCE_DTYPE array turned by `degrees` more (angles through atan2 in double, sin and cos rounded
    to float) and, where they translate, shifted by `shift`."""
    rec = records[np.asarray(indices)].copy()
    for k in range(len(rec)):
        d = degrees[k] if np.ndim(degrees) else degrees
        a = np.arctan2(float(rec["sin_t"][k]), float(rec["cos_t"][k])) + np.radians(d)
        rec["sin_t"][k], rec["cos_t"][k] = np.sin(a), np.cos(a)
        rec["flags"][k] |= ROTATE_Y
        if rec["flags"][k] & TRANSLATE:
            rec["offset"][k] += np.asarray(shift, F)
    return rec


def shows_moved(inst, prim, media, n_instances, moved_indices):
    """Pixels whose step 1a' instance is one of `moved_indices`."""
    return np.isin(followed_instance(inst, prim, n_instances, media), np.asarray(moved_indices))
