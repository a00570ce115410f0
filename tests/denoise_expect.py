"""What rt_denoise must return: the filter of include/rt_abi.h ("denoiser") restated in NumPy float32.

Every intermediate is an np.float32 array, every written operation is one NumPy operation (rounded once, nothing fused),
sums run left to right; the 25 taps are a Python loop in the contract's order (dy outer, dx inner), vectorised over the
image.  A tap outside the image leaves W and S of that pixel as they are.  The device result equals this bit for bit.

Also here, shared by the host and the GPU tests: seeded synthetic inputs (positive colours, unit and non-unit normals,
depths with zeros) and the oracle-side frames of tests/aov_expect.py (the oracle's noisy frame with the oracle-side
feature buffers).
"""
from __future__ import annotations

import numpy as np

F = np.float32
H = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]
ALBEDO_FLOOR = F(2.0 ** -10)
TINY = F(1e-20)
# the binding's keyword defaults (accelerated_ray_tracer_amd.DENOISE_DEFAULTS must say the same: tests/test_denoise_host.py)
DEFAULTS = dict(iterations=5, normal_sharpness=4, sigma_depth=0.2, sigma_color=2.0, color_floor=0.01)


def _shift(a, s, dx, dy):
    """a[j + s dy, i + s dx] where that is inside the image, and the mask of where it is; outside: zeros (never used)."""
    ny, nx = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((ny, nx), bool)
    ox, oy = s * dx, s * dy
    j0, j1 = max(0, -oy), min(ny, ny - oy)
    i0, i1 = max(0, -ox), min(nx, nx - ox)
    if j0 < j1 and i0 < i1:
        out[j0:j1, i0:i1] = a[j0 + oy:j1 + oy, i0 + ox:i1 + ox]
        ok[j0:j1, i0:i1] = True
    return out, ok


def denoise(color, albedo=None, normal=None, depth=None, *, iterations, sigma_color, color_floor, normal_sharpness, sigma_depth,
            demodulate=None, steps=None):
    """color (ny, nx, 3), albedo / normal (ny, nx, 3) or None, depth (ny, nx) or None -> (ny, nx, 3) float32.
    steps: None (the contract: s = 2^k), or the tap spacing of each iteration -- for tests that ask what a wrong one would do."""
    color = np.asarray(color, F)
    if demodulate is None:
        demodulate = albedo is not None
    sigma_color, color_floor, sigma_depth = F(sigma_color), F(color_floor), F(sigma_depth)
    with np.errstate(all="ignore"):
        if demodulate:
            a = np.fmax(np.asarray(albedo, F), ALBEDO_FLOOR)
            x = color / a
        else:
            x = color.copy()
        normal_on = normal is not None and normal_sharpness > 0
        depth_on = depth is not None and sigma_depth > 0
        color_on = sigma_color > 0
        N = np.asarray(normal, F) if normal_on else None
        Z = np.asarray(depth, F) if depth_on else None
        for k in range(iterations):
            s = 1 << k if steps is None else steps[k]
            sck = sigma_color * F(2.0 ** -k)
            W = np.zeros(x.shape[:2], F)
            S = np.zeros(x.shape, F)
            sp = (x[..., 0] + x[..., 1]) + x[..., 2]
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    xq, ok = _shift(x, s, dx, dy)
                    w = np.full(x.shape[:2], H[dy + 2] * H[dx + 2], F)
                    if dx or dy:
                        if normal_on:
                            Nq, _ = _shift(N, s, dx, dy)
                            d = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                            d = np.fmax(d, F(0))
                            for _ in range(normal_sharpness):
                                d = d * d
                            w = w * d
                        if depth_on:
                            Zq, _ = _shift(Z, s, dx, dy)
                            den = sigma_depth * np.fmax(Z, Zq) + TINY
                            r = np.abs(Z - Zq) / den
                            t = np.fmax(F(1) - r, F(0))
                            w = w * (t * t)
                        if color_on:
                            sq = (xq[..., 0] + xq[..., 1]) + xq[..., 2]
                            d1 = (np.abs(x[..., 0] - xq[..., 0]) + np.abs(x[..., 1] - xq[..., 1])) + np.abs(x[..., 2] - xq[..., 2])
                            den = sck * ((sp + sq) + color_floor)
                            r = d1 / den
                            t = np.fmax(F(1) - r, F(0))
                            w = w * (t * t)
                    assert w.dtype == F
                    W = np.where(ok, W + w, W)
                    S = np.where(ok[..., None], S + w[..., None] * xq, S)
            x = S / W[..., None]
            assert x.dtype == F
        return (x * a).astype(F) if demodulate else x


def synthetic(nx, ny, seed):
    """Seeded inputs: positive colours with a few bright pixels, albedo in [2^-12, 1] (some below the floor), normals that
    are unit in the left half and of any length up to 1 in the right (a few exactly zero, as on a miss), depths with zeros."""
    rng = np.random.default_rng(seed)
    albedo = rng.uniform(2.0 ** -12, 1.0, (ny, nx, 3)).astype(F)
    light = rng.uniform(0.05, 2.0, (ny, nx, 3)).astype(F)
    light[rng.random((ny, nx)) < 0.05] *= F(20)
    color = (albedo * light).astype(F)
    n = rng.normal(size=(ny, nx, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    n[:, nx // 2:] *= rng.random((ny, nx - nx // 2, 1))
    n[rng.random((ny, nx)) < 0.1] = 0
    # piecewise-smooth guides as well, so that not every weight is zero: blocks of 5 x 4 pixels share a normal and a depth
    by, bx = np.arange(ny)[:, None] // 4, np.arange(nx)[None, :] // 5
    blocky = rng.random((ny, nx)) < 0.6
    n[blocky] = n[(by * 4).clip(0, ny - 1), (bx * 5).clip(0, nx - 1)][blocky]
    depth = rng.uniform(0.5, 30.0, (ny, nx))
    depth[blocky] = (depth[(by * 4).clip(0, ny - 1), (bx * 5).clip(0, nx - 1)] * rng.uniform(0.98, 1.02, (ny, nx)))[blocky]
    depth[rng.random((ny, nx)) < 0.1] = 0
    return {"color": color, "albedo": albedo, "normal": n.astype(F), "depth": depth.astype(F)}


def reach(iterations):
    """How far, each way, one input pixel can be felt in the output: the sum of 2 s over the iterations."""
    return 2 * ((1 << iterations) - 1)


FLAT_COLOR, FLAT_ALBEDO = (0.5, 0.25, 0.125), (0.5, 0.5, 0.25)


def flat_regions(nx, ny):
    """(black, flat) of synthetic_flat: (j0, j1, i0, i1) of the 3 x 5 block of black pixels and of the flat region."""
    return (ny // 3, ny // 3 + 3, nx // 4, nx // 4 + 5), (ny // 2, min(ny, ny // 2 + 12), nx // 2, min(nx, nx // 2 + 16))


def synthetic_flat(nx, ny, seed):
    """synthetic()'s frame with what its random fields never hold.  The normal and the depth are exactly constant on blocks
    of 7 x 6 pixels, without jitter (a tenth of the blocks at depth 0), so that the depth factor is exactly 1 inside a block
    however small sigma_depth is.  A 3 x 5 block and six isolated pixels are exactly black, as in a few-sample frame of a
    dark scene: between two of them the colour factor's denominator is sigma times the floor alone.  And a region of 12 x 16
    pixels has one colour and one albedo, so that a tap pair there differs by exactly 0."""
    s = synthetic(nx, ny, seed)
    rng = np.random.default_rng(seed + 5)
    by, bx = np.arange(ny)[:, None] // 6, np.arange(nx)[None, :] // 7
    bn = rng.normal(size=(by.max() + 1, bx.max() + 1, 3))
    bn /= np.linalg.norm(bn, axis=2, keepdims=True)
    bz = rng.uniform(0.5, 30.0, bn.shape[:2])
    bz[rng.random(bz.shape) < 0.1] = 0
    s["normal"], s["depth"] = np.ascontiguousarray(bn[by, bx], F), np.ascontiguousarray(bz[by, bx], F)
    (j0, j1, i0, i1), (fj0, fj1, fi0, fi1) = flat_regions(nx, ny)
    s["color"][fj0:fj1, fi0:fi1], s["albedo"][fj0:fj1, fi0:fi1] = F(FLAT_COLOR), F(FLAT_ALBEDO)
    s["color"][j0:j1, i0:i1] = 0
    s["color"][rng.integers(0, ny, 6), rng.integers(0, nx, 6)] = 0
    return s


def synthetic_smooth(nx, ny, seed):
    """A frame in which taps hundreds of pixels apart still carry weight, as on one evenly lit wall: the light is one colour
    with 20 % noise per pixel, the normal one direction with a jitter of N(0, 0.02), the depth 10 within 3 %; the albedo is
    synthetic()'s.  (On synthetic()'s random blocks a far tap's weight is 0 or rounds away.)"""
    rng = np.random.default_rng(seed + 9)
    albedo = synthetic(nx, ny, seed)["albedo"]
    light = np.array([1.0, 0.7, 0.4]) * rng.uniform(0.8, 1.2, (ny, nx, 3))
    n = np.array([0.36, 0.48, 0.8]) + rng.normal(0.0, 0.02, (ny, nx, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    depth = 10.0 * rng.uniform(0.97, 1.03, (ny, nx))
    return {"color": (albedo * light).astype(F), "albedo": albedo, "normal": n.astype(F), "depth": depth.astype(F)}


def oracle_frame(art, orc, key, ns=4, nx=None, ny=None):
    """The oracle-side inputs of one tests/aov_expect.py scene: the oracle's ns-sample frame at gamma 1 and seed aov_expect.SEED
    as the noisy colour, and the oracle-side feature buffers (ns = min(ns, 16)), as DeviceScene.render_denoised pairs them."""
    import aov_expect as ax
    nx, ny = nx or ax.NX, ny or ax.NY
    c = ax.Case(art, orc, key)
    whole = orc.OracleScene.from_host(c.scene, nx, ny)
    color, _ = whole.render(ns, gamma=1.0, seed_base=ax.SEED)
    e = ax.expected(orc, c.scene, nx, ny, min(ns, 16), art, whole, c.twin)
    return {"color": color, "albedo": e["albedo"], "normal": e["normal"], "depth": e["depth"], "case": c, "oracle": whole}
