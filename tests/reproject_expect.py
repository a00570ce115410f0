"""What rt_reproject and its three extensions must return: the one NumPy restatement of the contract in include/rt_abi.h ("temporal
reprojection", "... that follows moved spheres", "... moved instances", "... moved quads and boxes").  reproject() writes steps 1 to
4 once; the sphere, instance and quad carries are parts of step 1 that run when their tables are given.  The record layouts and the
contract's helpers (which record a pixel follows, when two records differ, the maps and the carries) are here too;
tests/reproject_moving_expect.py, reproject_instances_expect.py and reproject_quads_expect.py call it the way their entries are called
and hold their inputs.

The matrix is formed in float64 from the camera's float32 fields; everything else is float32 with one rounding per written
operation (NumPy rounds every elementwise float32 operation once and never fuses two).  min and max are fmin and fmax: the
other operand when one is a NaN, as the device's are.  The four taps are visited in the contract's order, so the sums W, C
and L are taken left to right as written.

Also here, shared by the host and the GPU tests: the seeded synthetic buffers of the parity test and the cameras that go
with them, so that the properties which keep the test from testing nothing are checked on the very inputs the GPU test uses.
"""
from __future__ import annotations

import numpy as np

import scene_gen as sg

DEFAULTS = {"alpha_min": 0.5, "depth_tol": 0.05, "normal_min": 0.5, "max_history": 32.0}
F = np.float32


def _f3(v):
    return np.array([v[0], v[1], v[2]], np.float32)


def matrix(cam):
    """rt_reproject_matrix: float32 (3, 3), or None where the contract refuses the camera (D == 0, a non-finite entry)."""
    O, LL = _f3(cam.origin).astype(np.float64), _f3(cam.lower_left_corner).astype(np.float64)
    H, V = _f3(cam.horizontal).astype(np.float64), _f3(cam.vertical).astype(np.float64)
    A = LL - O

    def cross(x, y):
        return np.array([x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]], np.float64)
    r = [cross(H, V), cross(V, A), cross(A, H)]
    D = (A[0] * r[0][0] + A[1] * r[0][1]) + A[2] * r[0][2]
    if D == 0.0:
        return None
    with np.errstate(all="ignore"):
        m = np.array([[r[k][c] / D for c in range(3)] for k in range(3)], np.float64).astype(np.float32)
    return m if np.isfinite(m).all() else None


# ------------------------------------------------------------------------------------------------ records and helpers
SPHERE_DTYPE = np.dtype([("c0", "<f4", 3), ("radius", "<f4"), ("vel", "<f4", 3), ("mat", "<i4")])
MEDIUM_DTYPE = np.dtype([("boundary", "<i4"), ("neg_inv_density", "<f4"), ("mat", "<i4"), ("pad", "<i4")])
INSTANCE_DTYPE = np.dtype([("sin_t", "<f4"), ("cos_t", "<f4"), ("offset", "<f4", 3), ("child", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
QUAD_DTYPE = np.dtype([("Q", "<f4", 3), ("D", "<f4"), ("u", "<f4", 3), ("mat", "<i4"), ("v", "<f4", 3), ("pad0", "<f4"),
                       ("w", "<f4", 3), ("pad1", "<f4"), ("n", "<f4", 3), ("pad2", "<f4")])
SPHERE, QUAD, BOX, INSTANCE, MEDIUM = range(5)
ROTATE_Y, TRANSLATE = 1, 2


def ref(kind, index):
    """RT_PRIM_REF as an int32."""
    return int(np.array((kind << 28) | index, np.uint32).view(np.int32))


def shutter_centre(cam):
    """The binding's default for time / prev_time."""
    return F(0.5 * (cam.time0 + cam.time1))


def _mul(a, b):
    return (a * b).astype(F)


def dot(a, b):
    """The header's dot: (a.x b.x + a.y b.y) + a.z b.z; a, b: (..., 3) or a (3,) row."""
    return ((_mul(a[..., 0], b[..., 0]) + _mul(a[..., 1], b[..., 1])).astype(F) + _mul(a[..., 2], b[..., 2])).astype(F)


def cross(x, y):
    """The header's cross: (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0)."""
    return np.stack([(_mul(x[..., 1], y[..., 2]) - _mul(x[..., 2], y[..., 1])).astype(F),
                     (_mul(x[..., 2], y[..., 0]) - _mul(x[..., 0], y[..., 2])).astype(F),
                     (_mul(x[..., 0], y[..., 1]) - _mul(x[..., 1], y[..., 0])).astype(F)], axis=-1)


def _kind_index(refs):
    r = refs.astype(np.int64)
    return r, (r & 0xFFFFFFFF) >> 28, r & 0x0FFFFFFF


def _boundaries(prim, media):
    """(pixels that show a medium of `media`, that medium's boundary) -- the one record step 1a loads."""
    r, kind, index = _kind_index(prim)
    in_medium = (r >= 0) & (kind == MEDIUM) & (index < len(media))
    return in_medium, media["boundary"][np.where(in_medium, index, 0)]


def followed_sphere(prim, n_spheres, media):
    """Step 1a: the sphere index each pixel follows, or -1 (static)."""
    r, kind, index = _kind_index(prim)
    k = np.where((r >= 0) & (kind == SPHERE), index, -1)
    if media is not None and len(media):
        in_medium, boundary = _boundaries(prim, media)
        b, bkind, bindex = _kind_index(boundary)
        k = np.where(in_medium & (b >= 0) & (bkind == SPHERE), bindex, k)
    return np.where(k < n_spheres, k, -1)


def followed_instance(inst, prim, n_instances, media):
    """Step 1a': the instance index each pixel follows, or -1 (none: steps 1a-1c of rt_reproject_moving apply)."""
    ii = inst.astype(np.int64)
    i = np.where(ii >= 0, ii, -1)
    if media is not None and len(media):
        in_medium, boundary = _boundaries(prim, media)
        b, bkind, bindex = _kind_index(boundary)
        i = np.where((ii < 0) & in_medium & (b >= 0) & (bkind == INSTANCE), bindex, i)
    return np.where((i >= 0) & (i < n_instances), i, -1)


def followed_quad(prim, inst, n_quads, n_instances):
    """Step 1a'': the quad index each pixel follows, or -1 (none: rt_reproject_instances' step 1 applies unchanged)."""
    r, kind, index = _kind_index(prim)
    ii = inst.astype(np.int64)
    return np.where((r >= 0) & (kind == QUAD) & (index < n_quads) & ((ii < 0) | (ii < n_instances)), index, -1)


def carry_on_sphere(P, S, T, time, prev_time):
    """Steps 1b, 1c: (P', moved) for points P (..., 3) on the sphere records S (current) and T (previous): a NaN compares as moved."""
    with np.errstate(all="ignore"):
        cc = np.stack([(S["c0"][..., c] + _mul(time, S["vel"][..., c])).astype(F) for c in range(3)], axis=-1)
        cp = np.stack([(T["c0"][..., c] + _mul(prev_time, T["vel"][..., c])).astype(F) for c in range(3)], axis=-1)
        ratio = (T["radius"] / S["radius"]).astype(F)
        carried = np.stack([(cp[..., c] + _mul((P[..., c] - cc[..., c]).astype(F), ratio)).astype(F) for c in range(3)], axis=-1)
        return carried, (cc != cp).any(axis=-1) | (S["radius"] != T["radius"])


def records_differ(I, J):
    """Step 1b': a NaN compares as moved; child and pad are not looked at."""
    with np.errstate(all="ignore"):
        return (I["sin_t"] != J["sin_t"]) | (I["cos_t"] != J["cos_t"]) | (I["offset"] != J["offset"]).any(axis=-1) | (I["flags"] != J["flags"])


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


def to_object(P, I):
    """A and B of step 1c': world -> object by the current instance record."""
    with np.errstate(all="ignore"):
        return rotate_in(np.where(((I["flags"] & TRANSLATE) != 0)[..., None], (P - I["offset"]).astype(F), P).astype(F), I)


def to_world(B, J):
    """C and P' of step 1c': object -> previous world by the previous instance record."""
    with np.errstate(all="ignore"):
        C = rotate_out(B, J)
        return np.where(((J["flags"] & TRANSLATE) != 0)[..., None], (C + J["offset"]).astype(F), C).astype(F)


def carry_on_instance(P, I, J):
    """Step 1c' for the point: P (..., 3) float32, I and J records broadcastable against P's leading shape."""
    return to_world(to_object(P, I), J)


def turn_with_instance(N, I, J):
    """Step 1c' for the normal: the same two rotations, no translation."""
    return rotate_out(rotate_in(N, I), J)


def quad_records_differ(G, H):
    """Step 1b'': any component of Q, u or v compares != (a NaN compares as moved); D, w, n, mat and the pads do not enter."""
    with np.errstate(all="ignore"):
        return (G["Q"] != H["Q"]).any(axis=-1) | (G["u"] != H["u"]).any(axis=-1) | (G["v"] != H["v"]).any(axis=-1)


def planar(B, G):
    """(alpha, beta) of the object-space point B in the current record's frame: quad::hit's planar coordinates, not clamped."""
    with np.errstate(all="ignore"):
        h = (B - G["Q"]).astype(F)
        return dot(G["w"], cross(h, G["v"])), dot(G["w"], cross(G["u"], h))


def carry_on_quad(B, G, H):
    """Step 1c'' in object space: B (..., 3) float32 on the current record G -> B' on the previous record H."""
    with np.errstate(all="ignore"):
        a, b = planar(B, G)
        return np.stack([((H["Q"][..., c] + _mul(a, H["u"][..., c])).astype(F) + _mul(b, H["v"][..., c])).astype(F) for c in range(3)], axis=-1)


def normal_on_quad(Nb, G, H):
    """Step 1c'' for the object-space normal: the previous record's n, on the side and with the length the pixel saw."""
    with np.errstate(all="ignore"):
        s = dot(Nb, G["n"])
        return np.stack([_mul(s, H["n"][..., c]) for c in range(3)], axis=-1)


def _pair(cur, prev):
    """The length of a table of both frames (None: no table, 0)."""
    n = 0 if cur is None else len(cur)
    assert n == (0 if prev is None else len(prev)), "the tables of both frames have one length"
    return n


# ------------------------------------------------------------------------------------------------------ the contract
def reproject(color, depth, alpha, cur, prev, normal=None, prim=None, history=None, history_len=None, prev_depth=None,
              prev_alpha=None, prev_normal=None, prev_prim=None, spheres=None, prev_spheres=None, media=None, time=None, prev_time=None,
              inst=None, prev_inst=None, instances=None, prev_instances=None, quads=None, prev_quads=None,
              alpha_min=DEFAULTS["alpha_min"], depth_tol=DEFAULTS["depth_tol"], normal_min=DEFAULTS["normal_min"],
              max_history=DEFAULTS["max_history"], details=None):
    """-> (out (ny, nx, 3), out_len (ny, nx), motion (ny, nx, 2)), all float32: steps 1 to 4 of rt_reproject with, in step 1, the
    carries of the three extensions, each of which runs when its tables are given and moves nothing without a differing record.
    spheres / prev_spheres (SPHERE_DTYPE), instances / prev_instances (INSTANCE_DTYPE), quads / prev_quads (QUAD_DTYPE): arrays of
    one length per pair (None: no table); media: MEDIUM_DTYPE or None.  The prim test of a tap is on with history, prim and
    prev_prim; the inst test exactly when `inst` is passed, and the instance and quad tables need it.  details: a dict that receives
    "instance" (step 1a'), "on_instance" (surface pixels on the instance path), "followed" (those that took step 1c'), "quad" (step
    1a''), "on_quad", "followed_quad" (step 1c''), "under_instance" (quad-path pixels with an instance in range), "sphere" (step 1a,
    -1 on the instance path) and "followed_sphere" (pixels that took step 1c)."""
    assert inst is not None or (instances is None and quads is None), "the instance and quad tables need inst"
    ny, nx = depth.shape
    alpha_min, depth_tol, normal_min, max_history = F(alpha_min), F(depth_tol), F(normal_min), F(max_history)
    time = shutter_centre(cur) if time is None else F(time)
    prev_time = shutter_centre(prev) if prev_time is None else F(prev_time)
    n_spheres, n_instances, n_quads = _pair(spheres, prev_spheres), _pair(instances, prev_instances), _pair(quads, prev_quads)
    M = matrix(prev)
    assert M is not None, "the contract refuses this previous camera"
    normals_on = history is not None and normal is not None and prev_normal is not None
    ids_on = history is not None and prim is not None and prev_prim is not None
    O, LL, H, V, Op = _f3(cur.origin), _f3(cur.lower_left_corner), _f3(cur.horizontal), _f3(cur.vertical), _f3(prev.origin)
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
        qs, nrm = from_prev(P), normal
        none = np.full((ny, nx), -1, np.int64)
        # 1a' - 1c'. surface pixels on an instance whose record changed are carried back, their normals with them
        i = followed_instance(inst, prim, n_instances, media) if inst is not None else none
        has_i = (i >= 0)[..., None]
        records = lambda table: table[np.where(i >= 0, i, 0)] if n_instances else np.zeros((ny, nx), INSTANCE_DTYPE)   # noqa: E731
        I, J = records(instances), records(prev_instances)
        followed = surface & (i >= 0) & records_differ(I, J)
        qs = np.where(followed[..., None], from_prev(carry_on_instance(P, I, J)), qs).astype(F)
        if normals_on:
            nrm = np.where(followed[..., None], turn_with_instance(normal, I, J), normal).astype(F)
        # 1a'' - 1c''. surface pixels on a quad whose Q, u or v changed: in the instance's object space when there is one
        g = followed_quad(prim, inst, n_quads, n_instances) if n_quads else none
        followed_q = np.zeros((ny, nx), bool)
        if n_quads:
            G, Hq = quads[np.where(g >= 0, g, 0)], prev_quads[np.where(g >= 0, g, 0)]
            followed_q = surface & (g >= 0) & quad_records_differ(G, Hq)
            Bp = carry_on_quad(np.where(has_i, to_object(P, I), P).astype(F), G, Hq)
            qs = np.where(followed_q[..., None], from_prev(np.where(has_i, to_world(Bp, J), Bp).astype(F)), qs).astype(F)
            if normals_on:
                Nbp = normal_on_quad(np.where(has_i, rotate_in(normal, I), normal).astype(F), G, Hq)
                nrm = np.where(followed_q[..., None], np.where(has_i, rotate_out(Nbp, J), Nbp), nrm).astype(F)
        # 1a - 1c. every other surface pixel on a sphere whose record changed, or in a medium such a sphere bounds
        k = np.where(i >= 0, -1, followed_sphere(prim, n_spheres, media)) if n_spheres else none
        followed_s = np.zeros((ny, nx), bool)
        if n_spheres:
            carried, moved = carry_on_sphere(P, spheres[np.where(k >= 0, k, 0)], prev_spheres[np.where(k >= 0, k, 0)], time, prev_time)
            followed_s = surface & (k >= 0) & moved
            qs = np.where(followed_s[..., None], from_prev(carried), qs).astype(F)
        if details is not None:
            details.update(instance=i, on_instance=surface & (i >= 0), followed=followed, sphere=k, followed_sphere=followed_s,
                           quad=g, on_quad=surface & (g >= 0), followed_quad=followed_q, under_instance=surface & (g >= 0) & (i >= 0))
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
        # 3. the four taps, in order; every index is formed only where `window` holds and the tap is inside the image
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
            counts = inside & (hl > 0) & np.where(surface, geo, pa < alpha_min)
            if ids_on:
                counts &= prim == prev_prim[sy, sx]
            if inst is not None:
                counts &= inst == prev_inst[sy, sx]
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
def pinhole(lookfrom, lookat=(0.0, 0.0, 0.0), vfov=40.0, aspect=1.5, focus_dist=1.0):
    return sg.make_camera(lookfrom, lookat, vfov, aspect, 0.0, focus_dist, 0.0, 0.0)


def synthetic(nx, ny, seed):
    """Seeded buffers of two frames for the parity test: a current frame of two depth planes and some sky, a previous frame
    with the same structure shifted a little, history lengths with zeros among them, NaN and infinities in both depths, and
    three previous cameras -- "near" (a few degrees away: most pixels find their history), "same" and "behind" (in front of the
    points and looking away from them, so that a <= 0 for every surface pixel)."""
    rng = np.random.default_rng(seed)
    cur = pinhole((0.3, 0.2, 6.0), aspect=nx / ny)
    cams = {"near": pinhole((0.55, 0.15, 5.9), aspect=nx / ny), "same": pinhole((0.3, 0.2, 6.0), aspect=nx / ny),
            "behind": pinhole((0.0, 0.0, -40.0), lookat=(0.0, 0.0, -80.0), aspect=nx / ny)}

    def frame(shift):
        jj, ii = np.mgrid[0:ny, 0:nx]
        plane = np.where((ii + shift + jj // 3) % 11 < 6, 5.2, 6.9)
        depth = (plane + rng.uniform(-0.05, 0.05, (ny, nx))).astype(F)
        alpha = np.ones((ny, nx), F)
        sky = rng.random((ny, nx)) < 0.15
        alpha[sky], depth[sky] = 0.0, 0.0
        part = rng.random((ny, nx)) < 0.1            # partly covered pixels on both sides of alpha_min = 0.5
        alpha[part] = rng.choice(np.array([0.25, 0.5, 0.75], F), int(part.sum()))
        depth[part] *= alpha[part]
        nrm = rng.normal(size=(ny, nx, 3))
        nrm[..., 2] += 2.0
        nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(F)
        prim = rng.integers(0, 3, (ny, nx)).astype(np.int32)
        prim[sky] = -1
        return depth, alpha, nrm, prim
    depth, alpha, normal, prim = frame(0)
    pdepth, palpha, pnormal, pprim = frame(1)
    for d in (depth, pdepth):
        bad = rng.choice(nx * ny, min(12, nx * ny), replace=False)
        d.reshape(-1)[bad[0::3]] = np.nan
        d.reshape(-1)[bad[1::3]] = np.inf
        d.reshape(-1)[bad[2::3]] = -np.inf
    hlen = rng.integers(1, 40, (ny, nx)).astype(F)
    hlen[rng.random((ny, nx)) < 0.1] = 0.0
    return {"cur": cur, "cams": cams,
            "buffers": dict(color=rng.uniform(0.0, 2.0, (ny, nx, 3)).astype(F), depth=depth, alpha=alpha, normal=normal, prim=prim,
                            history=rng.uniform(0.0, 2.0, (ny, nx, 3)).astype(F), history_len=hlen, prev_depth=pdepth,
                            prev_alpha=palpha, prev_normal=pnormal, prev_prim=pprim)}


def select(buffers, normals, ids, history=True):
    """The keyword arguments of reproject() for one combination of guides."""
    keep = ["color", "depth", "alpha"] + (["history", "history_len", "prev_depth", "prev_alpha"] if history else [])
    keep += (["normal", "prev_normal"] if normals else []) + (["prim", "prev_prim"] if ids else [])
    return {k: buffers[k] for k in keep}


# ------------------------------------------------------------------------------- cameras and scenes of the GPU tests
def orbit(origin, lookat, degrees):
    """`origin` rotated about the vertical axis through `lookat` (float64)."""
    o, c = np.asarray(origin, np.float64), np.asarray(lookat, np.float64)
    th = np.radians(degrees)
    d = o - c
    return c + np.array([np.cos(th) * d[0] + np.sin(th) * d[2], d[1], -np.sin(th) * d[0] + np.cos(th) * d[2]])


GEN_LOOKAT, GEN_VFOV, GEN_FOCUS = (0.0, 0.4, 0.0), 40.0, 9.0        # scene_gen._camera's constants


def orbited_gen_camera(scene, nx, ny, degrees):
    """The camera of a scene_gen scene (its lens and shutter kept) with its eye orbited by `degrees`."""
    c = scene.desc.camera
    eye = orbit(list(c.origin), GEN_LOOKAT, degrees)
    return sg.make_camera(eye, GEN_LOOKAT, GEN_VFOV, nx / ny, 2.0 * c.lens_radius, GEN_FOCUS, c.time0, c.time1)


class WithCamera:
    """Anything with HostScene's surface (a HostScene or a scene_gen.GenScene) under another camera: a copy of the description
    with `camera` in it; every array is the original's, which is kept alive here."""

    def __init__(self, art, scene, camera):
        self.original = scene
        self.name = getattr(scene, "name", "desc") + "/camera"
        self.desc = art.RtSceneDesc.from_buffer_copy(scene.desc)
        self.desc.camera = camera
        self.nx, self.ny, self.ns, self.gamma = scene.nx, scene.ny, scene.ns, scene.gamma
        self.background, self.use_gradient_bg = scene.background, scene.use_gradient_bg
        self.materials = scene.materials
        self.frame = lambda **kw: art.HostScene.frame(self, **kw)

    def close(self):
        pass
