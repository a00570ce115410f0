"""CPU oracle binding.  TEST INFRASTRUCTURE ONLY (see rt_oracle.cpp header).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this;
nothing in accelerated-ray-tracer_amd/ does.  The reference has no golden vectors and
cannot be built in this image; the oracle is pinned at 8-bit level against the output images
the reference holds (tests/test_reference_images.py) and by the counters SURVEY.md recorded
from the reference's own code (tests/golden/survey_pins.json).  Below 8 bits (fp32 bit-level
vs a CUDA build) parity is unpinned: no such output of the reference exists.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.dirname(os.path.realpath(__file__))
LIB_PATH = os.path.join(_DIR, "librt_oracle.so")
_lib = None

COUNTER_NAMES = ["rays", "box_tests", "sphere_tests", "quad_tests", "medium_calls", "box6_calls", "inst_calls", "samples"]
CENSUS_NAMES = ["list", "spheres", "moving_spheres", "quads", "boxes", "instances", "media", "lambertian", "metal",
                "dielectric", "light", "depth"]


def build() -> None:
    r = subprocess.run(["make", "-C", _DIR, "librt_oracle.so"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("oracle build failed:\n" + r.stdout + r.stderr)


def load(path: str):
    """A ctypes handle of its own on an oracle library, with the argument types declared.  lib() loads the committed text's
    library through this; tests/oracle_mutants.py loads planted errors built elsewhere, each beside the others."""
    L = C.CDLL(path)
    if not hasattr(L, "orc_math_sweep"):
        raise RuntimeError(f"{path} is out of date and could not be rebuilt (make -C oracle)")
    L.orc_scene_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.orc_scene_from_desc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float]
    L.orc_scene_defaults.restype = C.c_float
    L.orc_scene_defaults.argtypes = [C.c_int, C.c_void_p]
    L.orc_render.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int,
                             C.c_ulonglong, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.orc_xorwow.argtypes = [C.c_ulonglong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.orc_dump_nodes.argtypes = [C.c_int, C.c_void_p, C.c_int]
    L.orc_scene_census.argtypes = [C.c_int, C.c_void_p]
    L.orc_camera.argtypes = [C.c_int, C.c_void_p]
    L.orc_perlin_noise.restype = C.c_float
    L.orc_perlin_noise.argtypes = [C.c_float] * 3
    L.orc_perlin_turb.restype = C.c_float
    L.orc_perlin_turb.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int]
    L.orc_math_sweep.argtypes = [C.c_int, C.c_uint, C.c_longlong, C.c_float, C.c_void_p, C.c_int]
    L.orc_math_list.argtypes = [C.c_int, C.c_longlong] + [C.c_void_p] * 4 + [C.c_int]
    return L


def lib():
    global _lib
    if _lib is None:
        try:
            build()          # make: a no-op when the library is newer than rt_oracle.cpp and include/rt_abi.h
        except (RuntimeError, OSError):
            if not os.path.exists(LIB_PATH):
                raise        # (a read-only tree with a library already built is still usable)
        _lib = load(LIB_PATH)
    return _lib


def xorwow(seed: int, n: int):
    state = np.zeros(6, np.uint32)
    uni = np.zeros(n, np.float32)
    raw = np.zeros(n, np.uint32)
    lib().orc_xorwow(seed, n, state.ctypes.data, uni.ctypes.data, raw.ctypes.data)
    return state, uni, raw


# orc_math_sweep / orc_math_list: the function ids of include/rt_abi.h's RT_MATH_*, and the oracle's own MATH_POW5_PRODUCT
MATH_LOG, MATH_SIN, MATH_ACOS, MATH_ATAN2, MATH_POW, MATH_POW5, MATH_SQRT, MATH_RCP, MATH_DIV, MATH_MULADD, MATH_POW5_PRODUCT = range(11)


def math_sweep(fn: int, first: int, count: int, operand: float = 0.0, threads: int = 0) -> np.ndarray:
    """The twin of rt_debug_math_tests' sweep form through the oracle's own wrappers: fn over the words first .. first + count - 1
    taken as floats (operand: gamma for MATH_POW), one uint64 digest per block of 2^20 words counted from `first`."""
    digests = np.zeros((count + (1 << 20) - 1) >> 20, np.uint64)
    threads = threads or min(os.cpu_count() or 1, 16)
    if lib().orc_math_sweep(fn, first, count, operand, digests.ctypes.data, threads) != 0:
        raise ValueError("orc_math_sweep refuses these arguments")
    return digests


def math_list(fn: int, a, b=None, c=None, threads: int = 0) -> np.ndarray:
    """The twin of the list form: out[i] = fn(a[i], b[i], c[i]) in float32; b and c may be None where fn does not read them."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    b, c = (None if x is None else np.ascontiguousarray(x, np.float32).reshape(-1) for x in (b, c))
    assert all(x is None or len(x) == len(a) for x in (b, c))
    out = np.zeros(len(a), np.float32)
    threads = threads or min(os.cpu_count() or 1, 16)
    ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    if lib().orc_math_list(fn, len(a), ptr(a), ptr(b), ptr(c), ptr(out), threads) != 0:
        raise ValueError("orc_math_list refuses these arguments")
    return out


class OracleScene:
    def __init__(self, name: str, nx: int, ny: int, image=None, iw: int = 0, ih: int = 0):
        self._img = None if image is None else np.ascontiguousarray(image, np.uint8)
        ptr = None if self._img is None else self._img.ctypes.data
        self.h = lib().orc_scene_create(name.encode(), nx, ny, ptr, iw, ih)
        if self.h < 0:
            raise ValueError(f"oracle has no scene '{name}'")
        self.name, self.nx, self.ny = name, nx, ny
        self._read_defaults()

    @classmethod
    def from_desc(cls, desc, nx: int, ny: int, gamma: float = 2.2, background=(0.0, 0.0, 0.0), gradient: int = 0, name: str = "desc"):
        """orc_scene_from_desc: the oracle's object graph filled from an rt_scene_desc (a ctypes structure laid out as
        include/rt_abi.h, e.g. HostScene.desc), copied.  nx, ny: the frame render() draws; gamma, background, gradient: what
        the frame description carries.  trace() reports a material as its index in the description; nodes() numbers the
        leaves by position.  ValueError when the description is refused (a bad index or kind, a non-binary interior node)."""
        import ctypes
        self = cls.__new__(cls)
        self._img = None
        bg = np.ascontiguousarray(background, np.float32)
        self.h = lib().orc_scene_from_desc(ctypes.addressof(desc), bg.ctypes.data, int(gradient), float(gamma))
        if self.h < 0:
            raise ValueError("the oracle refuses this scene description")
        self.name, self.nx, self.ny = name, nx, ny
        self._read_defaults()
        return self

    @classmethod
    def from_host(cls, hs, nx=None, ny=None):
        """from_desc for anything with HostScene's surface: its description, frame size and frame defaults."""
        return cls.from_desc(hs.desc, hs.nx if nx is None else nx, hs.ny if ny is None else ny, hs.gamma, hs.background,
                             hs.use_gradient_bg, getattr(hs, "name", "desc"))

    def _read_defaults(self):
        d = np.zeros(7, np.float32)
        self.gamma = float(lib().orc_scene_defaults(self.h, d.ctypes.data))
        self.def_nx, self.def_ny, self.def_ns, self.gradient = int(d[0]), int(d[1]), int(d[2]), int(d[3])
        self.background = d[4:7].copy()

    def render(self, ns: int, gamma=None, seed_base: int = 1984, row0: int = 0, row1=None, threads: int = 0, counters: bool = True):
        """Full-frame layout float32[ny][nx][3] (row 0 = bottom); rows outside [row0,row1) stay zero."""
        row1 = self.ny if row1 is None else row1
        threads = threads or min(os.cpu_count() or 1, 16)
        fb = np.zeros((self.ny, self.nx, 3), np.float32)
        cnt = np.zeros(8, np.uint64)
        bg = np.ascontiguousarray(self.background, np.float32)
        lib().orc_render(self.h, fb.ctypes.data, self.nx, self.ny, ns, self.gamma if gamma is None else gamma, bg.ctypes.data,
                         self.gradient, seed_base, row0, row1, cnt.ctypes.data if counters else None, threads)
        return fb, dict(zip(COUNTER_NAMES, (int(x) for x in cnt)))

    def nodes(self) -> np.ndarray:
        n = lib().orc_dump_nodes(self.h, None, 0)
        out = np.zeros((n, 8), np.float32)
        lib().orc_dump_nodes(self.h, out.ctypes.data, n)
        return out

    def node_passes(self, ns: int, threads: int = 0) -> tuple:
        """Diagnostics: renders the frame at `ns` spp counting, per BVH node (depth-first pre-order, as nodes()), the box tests
        that passed.  Returns (passes per node, rays, box tests)."""
        L = lib()
        L.orc_node_stats_enable.argtypes = [C.c_int, C.c_int]
        L.orc_node_passes.argtypes = [C.c_int, C.c_void_p, C.c_int]
        L.orc_node_stats_enable(self.h, 1)
        try:
            _, cnt = self.render(ns, threads=threads)
            n = len(self.nodes())
            p = np.zeros(n, np.uint64)
            L.orc_node_passes(self.h, p.ctypes.data, n)
        finally:
            L.orc_node_stats_enable(self.h, 0)
        return p.astype(np.float64), cnt["rays"], cnt["box_tests"]

    def trace(self, o, d, tm=None, tmin: float = 0.001, tmax=None, threads: int = 0):
        """orc_trace_rays: obj_hit of the world for caller rays.  o, d: (N, 3) float32; tm, tmax: (N,) float32 or None (0 /
        FLT_MAX).  Returns (t, p, n, uv, mat): t FLT_MAX and zero records on a miss; mat is the index of the hit's material
        in the oracle's material list (not the product's numbering), -1 on a miss."""
        L = lib()
        L.orc_trace_rays.argtypes = [C.c_int, C.c_longlong] + [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 6 + [C.c_int]
        o, d = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (o, d))
        n = len(o)
        assert d.shape == (n, 3)
        tm = None if tm is None else np.ascontiguousarray(tm, np.float32).reshape(n)
        tmax = None if tmax is None else np.ascontiguousarray(tmax, np.float32).reshape(n)
        t, p, nn = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        uv, mat = np.zeros((n, 2), np.float32), np.zeros(n, np.int32)
        threads = threads or min(os.cpu_count() or 1, 16)
        ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        L.orc_trace_rays(self.h, n, ptr(o), ptr(d), ptr(tm), float(tmin), ptr(tmax), ptr(t), ptr(p), ptr(nn), ptr(uv), ptr(mat),
                         threads)
        return t, p, nn, uv, mat

    def census(self) -> dict:
        c = np.zeros(12, np.int32)
        lib().orc_scene_census(self.h, c.ctypes.data)
        return dict(zip(CENSUS_NAMES, (int(x) for x in c)))

    def camera(self) -> np.ndarray:
        c = np.zeros(21, np.float32)
        lib().orc_camera(self.h, c.ctypes.data)
        return c
