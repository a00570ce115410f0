"""What rt_reproject_moving must return: a NumPy restatement of the whole extended contract in include/rt_abi.h ("temporal
reprojection that follows moved spheres"): step 1 with its tail 1a-1c, then steps 2-4 of rt_reproject.

As in tests/reproject_expect.py everything but the matrix is float32 with one rounding per written operation, min and max are
fmin and fmax, and the four taps are visited in the contract's order.  Ids are required and the id test of a tap is always on.

Also here, shared by the host and the GPU tests: synthetic_moving(), the seeded buffers of the parity test with ids and tables
that reach every branch of the tail, so that the properties which keep the test from testing nothing are checked on the very
inputs the GPU test uses.
"""
from __future__ import annotations

import numpy as np

import reproject_expect as rx

F = np.float32
DEFAULTS = rx.DEFAULTS
SPHERE_DTYPE = np.dtype([("c0", "<f4", 3), ("radius", "<f4"), ("vel", "<f4", 3), ("mat", "<i4")])
MEDIUM_DTYPE = np.dtype([("boundary", "<i4"), ("neg_inv_density", "<f4"), ("mat", "<i4"), ("pad", "<i4")])
SPHERE, QUAD, BOX, INSTANCE, MEDIUM = range(5)


def ref(kind, index):
    """RT_PRIM_REF as an int32."""
    return int(np.array((kind << 28) | index, np.uint32).view(np.int32))


def shutter_centre(cam):
    """The binding's default for time / prev_time."""
    return F(0.5 * (cam.time0 + cam.time1))


def followed_sphere(prim, n_spheres, media):
    """Step 1a: the sphere index each pixel follows, or -1 (static)."""
    r = prim.astype(np.int64)
    kind, index = (r & 0xFFFFFFFF) >> 28, r & 0x0FFFFFFF
    k = np.full(prim.shape, -1, np.int64)
    k = np.where((r >= 0) & (kind == SPHERE), index, k)
    n_media = 0 if media is None else len(media)
    if n_media:
        in_medium = (r >= 0) & (kind == MEDIUM) & (index < n_media)
        b = media["boundary"][np.where(in_medium, index, 0)].astype(np.int64)
        k = np.where(in_medium & (b >= 0) & (((b & 0xFFFFFFFF) >> 28) == SPHERE), b & 0x0FFFFFFF, k)
    return np.where(k < n_spheres, k, -1)


def reproject(color, depth, alpha, cur, prev, normal=None, prim=None, history=None, history_len=None, prev_depth=None,
              prev_alpha=None, prev_normal=None, prev_prim=None, spheres=None, prev_spheres=None, media=None, time=None, prev_time=None,
              alpha_min=DEFAULTS["alpha_min"], depth_tol=DEFAULTS["depth_tol"], normal_min=DEFAULTS["normal_min"],
              max_history=DEFAULTS["max_history"], details=None):
    """-> (out (ny, nx, 3), out_len (ny, nx), motion (ny, nx, 2)), all float32.  spheres / prev_spheres: SPHERE_DTYPE arrays of one
    length (None: no table, n_spheres = 0); media: MEDIUM_DTYPE or None.  details: a dict that receives "followed" (ny, nx), the
    pixels that took step 1c, and "sphere", the result of step 1a."""
    assert prim is not None and prev_prim is not None, "ids are required"
    ny, nx = depth.shape
    alpha_min, depth_tol, normal_min, max_history = F(alpha_min), F(depth_tol), F(normal_min), F(max_history)
    time = shutter_centre(cur) if time is None else F(time)
    prev_time = shutter_centre(prev) if prev_time is None else F(prev_time)
    n_spheres = 0 if spheres is None else len(spheres)
    assert n_spheres == (0 if prev_spheres is None else len(prev_spheres))
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
        # 1a - 1c. surface pixels on a sphere whose record changed are carried back first
        k = followed_sphere(prim, n_spheres, media)
        followed = np.zeros((ny, nx), bool)
        if n_spheres:
            kk = np.where(k >= 0, k, 0)
            S, T = spheres[kk], prev_spheres[kk]
            cc = np.stack([(S["c0"][..., c] + (time * S["vel"][..., c]).astype(F)).astype(F) for c in range(3)], axis=-1)
            cp = np.stack([(T["c0"][..., c] + (prev_time * T["vel"][..., c]).astype(F)).astype(F) for c in range(3)], axis=-1)
            moved = (cc != cp).any(axis=-1) | (S["radius"] != T["radius"])
            followed = surface & (k >= 0) & moved
            ratio = (T["radius"] / S["radius"]).astype(F)
            carried = np.stack([(cp[..., c] + ((P[..., c] - cc[..., c]).astype(F) * ratio).astype(F)).astype(F) for c in range(3)], axis=-1)
            qm = np.stack([(carried[..., c] - Op[c]).astype(F) for c in range(3)], axis=-1)
            qs = np.where(followed[..., None], qm, qs).astype(F)
        if details is not None:
            details["followed"], details["sphere"] = followed, k
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
                geo &= dot(normal, prev_normal[sy, sx]) >= normal_min
            counts = inside & (hl > 0) & np.where(surface, geo, pa < alpha_min) & (prim == prev_prim[sy, sx])
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
N_SPHERES = 10
# what each record of the tables is there for (index -> reason); synthetic_moving builds them in this order
RECORDS = ["moved", "unmoved", "radius only", "previous radius 0", "current radius 0", "negative radius", "nan c0", "infinite vel",
           "velocity, time != prev_time", "moved further"]


def tables():
    """(spheres, prev_spheres, media, time, prev_time) of the parity test."""
    cur = np.zeros(N_SPHERES, SPHERE_DTYPE)
    cur["c0"] = np.array([0.1, -0.2, 0.4], F) + np.arange(N_SPHERES, dtype=F)[:, None] * np.array([0.05, 0.02, -0.03], F)
    cur["radius"] = 1.0
    cur["mat"] = np.arange(N_SPHERES)
    prev = cur.copy()
    prev["c0"][0] += np.array([0.06, -0.04, 0.02], F)                         # moved
    prev["radius"][2] = 0.9                                                    # radius only
    prev["radius"][3] = 0.0                                                    # previous radius 0: everything lands on the centre
    cur["radius"][4] = 0.0                                                     # current radius 0: a division by zero
    cur["radius"][5], prev["radius"][5] = -1.0, -1.25                          # negative radius (a flipped sphere)
    prev["c0"][5] += np.array([0.0, 0.03, 0.0], F)
    cur["c0"][6, 1] = np.nan                                                   # NaN compares as moved
    cur["vel"][7, 0] = np.inf                                                  # an infinite centre in the current frame only
    cur["vel"][8] = prev["vel"][8] = np.array([0.2, -0.1, 0.05], F)           # the same record in both frames, followed by time alone
    prev["c0"][9] += np.array([-0.3, 0.2, 0.1], F)
    prev["radius"][9] = 1.1
    media = np.zeros(6, MEDIUM_DTYPE)
    media["boundary"] = [ref(SPHERE, 0), ref(QUAD, 1), -1, ref(SPHERE, N_SPHERES), ref(SPHERE, 0x0FFFFFFF), ref(INSTANCE, 0)]
    media["neg_inv_density"] = -1.0
    return cur, prev, media, F(0.5), F(0.25)


def unmoved_tables():
    """Tables of the same shape in which no record moved: both frames hold the current records (the NaN replaced: a NaN compares
    as moved) at one instant."""
    cur, _, media, time, _ = tables()
    cur["c0"][6, 1] = 0.25
    return cur, cur.copy(), media, time, time


def id_palette():
    """The ids the synthetic frames are painted with: every branch of step 1a."""
    n_media = 6
    return np.array([-1, ref(SPHERE, 0), ref(SPHERE, 1), ref(SPHERE, 2), ref(SPHERE, 3), ref(SPHERE, 4), ref(SPHERE, 5), ref(SPHERE, 6),
                     ref(SPHERE, 7), ref(SPHERE, 8), ref(SPHERE, 9), ref(SPHERE, N_SPHERES), ref(SPHERE, 0x0FFFFFFF), ref(QUAD, 0), ref(QUAD, 3),
                     ref(MEDIUM, 0), ref(MEDIUM, 1), ref(MEDIUM, 2), ref(MEDIUM, 3), ref(MEDIUM, 4), ref(MEDIUM, 5), ref(MEDIUM, n_media),
                     ref(MEDIUM, 0x0FFFFFFF), ref(BOX, 2), ref(5, 3), ref(7, 0x0FFFFFFF), -2147483648, -2], np.int32)


def synthetic_moving(nx, ny, seed):
    """rx.synthetic's buffers with prim / prev_prim painted over in small patches from id_palette() -- the same patches in both
    frames, with one pixel in eight of the previous frame repainted at random, so that taps pass and fail the id test -- and the
    tables of tables().  The moved sphere and the medium it bounds come up more often than the rest."""
    s = rx.synthetic(nx, ny, seed)
    rng = np.random.default_rng(seed + 1000)
    pal = id_palette()
    weights = np.ones(len(pal))
    weights[[1, 10, 15]] = 4.0
    jj, ii = np.mgrid[0:ny, 0:nx]
    patch = (ii // 3) + ((nx + 2) // 3) * (jj // 2)
    choice = rng.choice(len(pal), int(patch.max()) + 1, p=weights / weights.sum())
    if len(choice) >= len(pal):                      # every id at least once, wherever the frame has room for that
        choice[rng.permutation(len(choice))[:len(pal)]] = np.arange(len(pal))
    prim = pal[choice[patch]].astype(np.int32)
    prev_prim = prim.copy()
    again = rng.random((ny, nx)) < 0.125
    prev_prim[again] = pal[rng.integers(0, len(pal), int(again.sum()))]
    b = dict(s["buffers"], prim=prim, prev_prim=prev_prim)
    spheres, prev_spheres, media, time, prev_time = tables()
    return {"cur": s["cur"], "cams": s["cams"], "buffers": b,
            "tables": dict(spheres=spheres, prev_spheres=prev_spheres, media=media, time=time, prev_time=prev_time)}


def select(buffers, normals, history=True):
    """The keyword arguments of reproject() with the normal test on or off; ids always."""
    keep = ["color", "depth", "alpha", "prim", "prev_prim"] + (["history", "history_len", "prev_depth", "prev_alpha"] if history else [])
    keep += ["normal", "prev_normal"] if normals else []
    return {k: buffers[k] for k in keep}


# -------------------------------------------------------------------------------------- the real pair of the GPU test
# general_tex's direct spheres that the 64 x 48 frame shows, and what happens to them between the two frames
REAL_MOVE = np.array([0.0, 0.35, 0.0], F)
REAL_GROW = F(1.15)


def real_update(scene, count=6):
    """(indices, records): the `count` largest direct spheres of `scene` that are not its ground, lifted by REAL_MOVE, every other
    one also grown by REAL_GROW."""
    import refit_expect as rf
    sph = scene.spheres()
    direct = rf.direct_spheres(scene)
    direct = direct[np.abs(sph["radius"][direct]) < 100.0]
    idx = direct[np.argsort(-np.abs(sph["radius"][direct]), kind="stable")[:count]]
    rec = sph[idx]
    rec["c0"] += REAL_MOVE
    rec["radius"][::2] *= REAL_GROW
    return idx.astype(np.int32), rec
