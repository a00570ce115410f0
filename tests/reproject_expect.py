"""What rt_reproject must return: a NumPy restatement of the contract in include/rt_abi.h ("temporal reprojection").

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


def _dot(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z, float32; a, b: (..., 3) or a (3,) row."""
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def reproject(color, depth, alpha, cur, prev, normal=None, prim=None, history=None, history_len=None, prev_depth=None,
              prev_alpha=None, prev_normal=None, prev_prim=None, alpha_min=DEFAULTS["alpha_min"], depth_tol=DEFAULTS["depth_tol"],
              normal_min=DEFAULTS["normal_min"], max_history=DEFAULTS["max_history"]):
    """-> (out (ny, nx, 3), out_len (ny, nx), motion (ny, nx, 2)), all float32."""
    ny, nx = depth.shape
    alpha_min, depth_tol, normal_min, max_history = F(alpha_min), F(depth_tol), F(normal_min), F(max_history)
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
        qs = np.stack([(P[..., c] - Op[c]).astype(F) for c in range(3)], axis=-1)
        q = np.where(surface[..., None], qs, dirv).astype(F)
        # 2. into the previous camera
        a, b, c_ = _dot(M[0], q), _dot(M[1], q), _dot(M[2], q)
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
        for k in range(4):
            qx, qy = ix + (k & 1), iy + (k >> 1)
            inside = window & (qx >= 0) & (qx < nx) & (qy >= 0) & (qy < ny)
            sx, sy = np.where(inside, qx, 0), np.where(inside, qy, 0)
            hl, pa, pd = history_len[sy, sx], prev_alpha[sy, sx], prev_depth[sy, sx]
            zq = (pd / pa).astype(F)
            geo_surface = (pa >= alpha_min) & (np.abs((zq - a).astype(F)) <= (depth_tol * np.fmax(zq, a)).astype(F))
            if normals_on:
                geo_surface &= _dot(normal, prev_normal[sy, sx]) >= normal_min
            counts = inside & (hl > 0) & np.where(surface, geo_surface, pa < alpha_min)
            if ids_on:
                counts &= prim == prev_prim[sy, sx]
            w = weights[k]
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
