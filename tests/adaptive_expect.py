"""What rt_render_adaptive must return, predicted from CPU oracle renders alone (include/rt_abi.h, "adaptive sampling").

The oracle renders every pixel at any sample count; a pixel of an adaptive frame is the oracle's pixel at the count the
criterion chose for it.  The criterion is evaluated here in numpy float64 from the float32 averages, in the order the
header states, so that it reproduces the device's double arithmetic exactly.
"""
from __future__ import annotations

import ctypes as C

import numpy as np


def checkpoints(min_spp: int, max_spp: int) -> list:
    out, n = [], min_spp
    while n <= max_spp:
        out.append(n)
        n *= 2
    assert out[-1] == max_spp, (min_spp, max_spp)
    return out


def converged(a: np.ndarray, h: np.ndarray, threshold: float, floor: float) -> np.ndarray:
    """The criterion for float32 averages a, h of shape (..., 3): float64, left to right; NaN never converges."""
    if np.float32(threshold) < 0:
        return np.zeros(a.shape[:-1], bool)
    a64, h64 = a.astype(np.float64), h.astype(np.float64)
    d = np.abs(a64[..., 0] - h64[..., 0]) + np.abs(a64[..., 1] - h64[..., 1]) + np.abs(a64[..., 2] - h64[..., 2])
    s = a64[..., 0] + a64[..., 1] + a64[..., 2]
    with np.errstate(invalid="ignore"):
        return d <= np.float64(np.float32(threshold)) * (s + np.float64(np.float32(floor)))


def spp_map(linear: dict, min_spp: int, max_spp: int, threshold: float, floor: float) -> np.ndarray:
    """Final counts from the gamma-1 frames `linear[n]` for n = min/2 and every checkpoint."""
    cps = checkpoints(min_spp, max_spp)
    shape = linear[cps[0]].shape[:-1]
    spp = np.full(shape, max_spp, np.int32)
    active = np.ones(shape, bool)
    for n in cps[:-1]:
        stop = active & converged(linear[n], linear[n // 2], threshold, floor)
        spp[stop] = n
        active &= ~stop
    return spp


def pixel_rays(orc_scene, ns: int, seed_base: int = 1984) -> np.ndarray:
    """Rays of every pixel of a render at ns samples, full-frame layout [ny][nx] (orc_row_pixel_rays)."""
    L = orc_scene_lib()
    bg = np.ascontiguousarray(orc_scene.background, np.float32)
    out = np.zeros((orc_scene.ny, orc_scene.nx), np.uint64)
    row = np.zeros(orc_scene.nx, np.uint64)
    for j in range(orc_scene.ny):
        L.orc_row_pixel_rays(orc_scene.h, orc_scene.nx, orc_scene.ny, ns, bg.ctypes.data, orc_scene.gradient, seed_base, j, row.ctypes.data)
        out[j] = row
    return out


_bound = None


def orc_scene_lib():
    global _bound
    if _bound is None:
        import oracle
        L = oracle.lib()
        L.orc_row_pixel_rays.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_ulonglong, C.c_int, C.c_void_p]
        L.orc_row_pixel_rays.restype = None
        _bound = L
    return _bound


class Expectation:
    """Oracle renders of one scene and frame size, cached by sample count and gamma."""

    def __init__(self, orc_scene, seed_base: int = 1984):
        self.o, self.seed_base = orc_scene, seed_base
        self._frames, self._rays = {}, {}

    def frame(self, ns: int, gamma: float = 1.0) -> np.ndarray:
        key = (ns, float(np.float32(gamma)))
        if key not in self._frames:
            self._frames[key] = self.o.render(ns, gamma=gamma, seed_base=self.seed_base, counters=False)[0]
        return self._frames[key]

    def rays(self, ns: int) -> np.ndarray:
        if ns not in self._rays:
            self._rays[ns] = pixel_rays(self.o, ns, self.seed_base)
        return self._rays[ns]

    def spp(self, min_spp: int, max_spp: int, threshold: float, floor: float) -> np.ndarray:
        ns = [min_spp // 2] + checkpoints(min_spp, max_spp)
        return spp_map({n: self.frame(n) for n in ns if n > 0}, min_spp, max_spp, threshold, floor)

    def predict(self, min_spp: int, max_spp: int, threshold: float, floor: float, gamma: float = 1.0):
        """(fb, spp, rays, samples) of the whole frame, full-frame layout; rays / samples summed over every pixel."""
        spp = self.spp(min_spp, max_spp, threshold, floor)
        fb = np.zeros(spp.shape + (3,), np.float32)
        rays = np.zeros(spp.shape, np.uint64)
        for n in np.unique(spp):
            m = spp == n
            fb[m] = self.frame(int(n), gamma)[m]
            rays[m] = self.rays(int(n))[m]
        return fb, spp, rays, spp.astype(np.int64)

    def threshold_with_spread(self, min_spp: int, max_spp: int, floor: float, candidates=(0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 1.0, 0.01)):
        """The first candidate threshold under which at least three distinct counts occur (None if none does)."""
        for t in candidates:
            if len(np.unique(self.spp(min_spp, max_spp, t, floor))) >= 3:
                return t
        return None
