"""accelerated-ray-tracer_amd: MI355X-native render path of the reference path tracer.

Python is only plumbing here (tests, bench, torch.distributed glue).  The
product is two C libraries built from this directory:

* ``lib/librt_mi355x.so``  -- HIP kernels + the C ABI of ``include/rt_abi.h``
* ``lib/librtw_host.so``   -- host mirror of the reference's scene classes,
  scene builders, flattener, PPM writer

This module binds both with ctypes.  There is no CPU render fallback: if the
HIP library is missing or no gfx950 device is visible, rendering raises.

The directory name carries a hyphen (it follows the reference repository's
name); import it through the ``accelerated_ray_tracer_amd`` symlink.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.realpath(__file__))
REPO_ROOT = os.path.dirname(PKG_DIR)
LIB_DIR = os.path.join(PKG_DIR, "lib")
RT_LIB_PATH = os.environ.get("RT_LIB_OVERRIDE") or os.path.join(LIB_DIR, "librt_mi355x.so")   # override: diagnostic builds only
HOST_LIB_PATH = os.environ.get("RTW_LIB_OVERRIDE") or os.path.join(LIB_DIR, "librtw_host.so")   # override: experiments only


class RtError(RuntimeError):
    pass


# ----------------------------------------------------------------------------- structs of rt_abi.h
class RtCamera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("lower_left_corner", C.c_float * 3), ("horizontal", C.c_float * 3),
                ("vertical", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("lens_radius", C.c_float),
                ("pad", C.c_float), ("time0", C.c_double), ("time1", C.c_double)]


class RtSceneDesc(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("n_nodes", C.c_int32),
                ("spheres", C.c_void_p), ("n_spheres", C.c_int32),
                ("quads", C.c_void_p), ("n_quads", C.c_int32),
                ("boxes", C.c_void_p), ("n_boxes", C.c_int32),
                ("instances", C.c_void_p), ("n_instances", C.c_int32),
                ("media", C.c_void_p), ("n_media", C.c_int32),
                ("materials", C.c_void_p), ("n_materials", C.c_int32),
                ("textures", C.c_void_p), ("n_textures", C.c_int32),
                ("images", C.c_void_p), ("image_bytes", C.c_size_t),
                ("camera", RtCamera)]


class RtFrameDesc(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("ns", C.c_int32), ("gamma", C.c_float),
                ("background", C.c_float * 3), ("use_gradient_bg", C.c_int32), ("seed_base", C.c_uint64),
                ("tile_rows", C.c_int32), ("tile_first", C.c_int32), ("tile_stride", C.c_int32), ("reserved", C.c_int32)]


class RtStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("samples", C.c_uint64), ("ms_render", C.c_double), ("local_rows", C.c_int32),
                ("kernel_variant", C.c_int32), ("workgroups", C.c_int32), ("threads_per_group", C.c_int32),
                ("lds_bytes", C.c_int32), ("reserved", C.c_int32)]


class RtRayBatch(C.Structure):
    _fields_ = [("n", C.c_int64), ("origins", C.c_void_p), ("directions", C.c_void_p), ("times", C.c_void_p), ("tmax", C.c_void_p),
                ("tmin", C.c_float), ("mode", C.c_int32),
                ("t_out", C.c_void_p), ("prim_out", C.c_void_p), ("inst_out", C.c_void_p), ("point_out", C.c_void_p),
                ("normal_out", C.c_void_p), ("uv_out", C.c_void_p), ("mat_out", C.c_void_p), ("hit_out", C.c_void_p)]


class RtRadianceBatch(C.Structure):
    _fields_ = [("n", C.c_int64), ("origins", C.c_void_p), ("directions", C.c_void_p), ("times", C.c_void_p), ("seeds", C.c_void_p),
                ("seed_base", C.c_uint64), ("ns", C.c_int32), ("background", C.c_float * 3), ("use_gradient_bg", C.c_int32),
                ("reserved", C.c_int32), ("rgb_out", C.c_void_p), ("rays_out", C.c_void_p)]


class RtAovDesc(C.Structure):
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("alpha", C.c_void_p),
                ("prim", C.c_void_p), ("inst", C.c_void_p), ("mat", C.c_void_p)]


class RtAovThroughDesc(C.Structure):
    _fields_ = [("max_bounces", C.c_int32), ("fuzz_limit", C.c_float), ("through", C.c_void_p), ("bounces", C.c_void_p)]


class RtDenoiseDesc(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("color", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p),
                ("depth", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("iterations", C.c_int32), ("normal_sharpness", C.c_int32), ("demodulate", C.c_int32), ("reserved", C.c_int32),
                ("sigma_color", C.c_float), ("color_floor", C.c_float), ("sigma_depth", C.c_float), ("pad", C.c_float)]


class RtUpscaleDesc(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("factor", C.c_int32), ("normal_sharpness", C.c_int32), ("demodulate", C.c_int32),
                ("reserved", C.c_int32), ("sigma_depth", C.c_float), ("min_weight", C.c_float), ("color_lo", C.c_void_p),
                ("albedo_lo", C.c_void_p), ("normal_lo", C.c_void_p), ("depth_lo", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p),
                ("depth", C.c_void_p), ("out", C.c_void_p), ("weight_out", C.c_void_p)]


class RtAdaptiveDesc(C.Structure):
    _fields_ = [("min_spp", C.c_int32), ("max_spp", C.c_int32), ("threshold", C.c_float), ("floor", C.c_float)]


class RtVarianceDesc(C.Structure):
    _fields_ = [("batches", C.c_int32), ("reserved", C.c_int32)]


class RtDenoiseVarianceDesc(C.Structure):
    _fields_ = [("variance", C.c_void_p), ("variance_out", C.c_void_p), ("sigma_variance", C.c_float), ("variance_floor", C.c_float)]


class RtReprojectDesc(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("cur", RtCamera), ("prev", RtCamera),
                ("color", C.c_void_p), ("depth", C.c_void_p), ("alpha", C.c_void_p), ("normal", C.c_void_p), ("prim", C.c_void_p),
                ("history", C.c_void_p), ("history_len", C.c_void_p), ("prev_depth", C.c_void_p), ("prev_alpha", C.c_void_p),
                ("prev_normal", C.c_void_p), ("prev_prim", C.c_void_p), ("out", C.c_void_p), ("out_len", C.c_void_p), ("motion", C.c_void_p),
                ("alpha_min", C.c_float), ("depth_tol", C.c_float), ("normal_min", C.c_float), ("max_history", C.c_float)]


class RtReprojectMotionDesc(C.Structure):
    _fields_ = [("n_spheres", C.c_int32), ("n_media", C.c_int32), ("spheres", C.c_void_p), ("prev_spheres", C.c_void_p),
                ("media", C.c_void_p), ("time", C.c_float), ("prev_time", C.c_float)]


class RtReprojectInstanceDesc(C.Structure):
    _fields_ = [("n_instances", C.c_int32), ("reserved", C.c_int32), ("instances", C.c_void_p), ("prev_instances", C.c_void_p),
                ("inst", C.c_void_p), ("prev_inst", C.c_void_p)]


class RtReprojectQuadDesc(C.Structure):
    _fields_ = [("n_quads", C.c_int32), ("reserved", C.c_int32), ("quads", C.c_void_p), ("prev_quads", C.c_void_p)]


class RtSphereUpdate(C.Structure):
    _fields_ = [("count", C.c_int32), ("first", C.c_int32), ("indices", C.c_void_p), ("spheres", C.c_void_p)]


class RtInstanceUpdate(C.Structure):
    _fields_ = [("count", C.c_int32), ("first", C.c_int32), ("indices", C.c_void_p), ("instances", C.c_void_p)]


class RtQuadUpdate(C.Structure):
    _fields_ = [("count", C.c_int32), ("first", C.c_int32), ("indices", C.c_void_p), ("quads", C.c_void_p)]


RT_INST_ROTATE_Y, RT_INST_TRANSLATE = 1, 2
RT_TRACE_CLOSEST, RT_TRACE_ANY = 0, 1
RT_PRIM_SPHERE, RT_PRIM_QUAD, RT_PRIM_BOX, RT_PRIM_INSTANCE, RT_PRIM_MEDIUM = range(5)


def prim_kind(ref):
    """Kind of an RT_PRIM_REF (scalar or integer array); -1 refs (misses) give 15."""
    return (np.asarray(ref).astype(np.int64) & 0xFFFFFFFF) >> 28


def prim_index(ref):
    return np.asarray(ref).astype(np.int64) & 0x0FFFFFFF


# DeviceScene.trace(): closest hit -- the record fields are None unless record=True
TraceResult = collections.namedtuple("TraceResult", "t prim inst point normal uv mat")
# DeviceScene.render_aov(): the outputs of rt_render_aov -> (channels, numpy dtype)
AOV_OUTPUTS = {"albedo": (3, np.float32), "normal": (3, np.float32), "depth": (1, np.float32), "alpha": (1, np.float32),
               "prim": (1, np.int32), "inst": (1, np.int32), "mat": (1, np.int32)}
# DeviceScene.render_aov_through(): rt_render_aov's outputs and the two of rt_aov_through_desc
AOV_THROUGH_OUTPUTS = dict(AOV_OUTPUTS, through=(1, np.float32), bounces=(1, np.int32))
# ... and its keyword defaults; fuzz_limit settled on the oracle's 4-spp frames
AOV_THROUGH_DEFAULTS = {"max_bounces": 8, "fuzz_limit": 0.0}
# denoise(): the keyword defaults (they live here, not in the ABI); settled on the oracle's 4-spp frames
DENOISE_DEFAULTS = {"iterations": 5, "normal_sharpness": 4, "sigma_depth": 0.2, "sigma_color": 2.0, "color_floor": 0.01}
# denoise(variance=...): the keyword defaults of the variance factor, settled by a sweep on the same frames
DENOISE_VARIANCE_DEFAULTS = {"sigma_variance": 3.0, "variance_floor": 1e-4}
# upscale(): the keyword defaults
UPSCALE_DEFAULTS = dict(normal_sharpness=4, sigma_depth=0.2, min_weight=2**-6)
# reproject() / TemporalAccumulator: the keyword defaults of rt_reproject's four thresholds
REPROJECT_DEFAULTS = {"alpha_min": 0.5, "depth_tol": 0.05, "normal_min": 0.5, "max_history": 32.0}
# reproject(): out is the accumulated frame (the next call's history), length its per-pixel history length, motion the
# per-pixel offset into the previous frame (None unless motion=True)
ReprojectResult = collections.namedtuple("ReprojectResult", "out length motion")
# DeviceScene.radiance(): rays is None unless count_rays=True
RadianceResult = collections.namedtuple("RadianceResult", "rgb rays")

NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("skip", "<i4"), ("bmax", "<f4", 3), ("prim", "<i4")])
SPHERE_DTYPE = np.dtype([("c0", "<f4", 3), ("radius", "<f4"), ("vel", "<f4", 3), ("mat", "<i4")])
MATERIAL_DTYPE = np.dtype([("kind", "<i4"), ("tex", "<i4"), ("fuzz", "<f4"), ("ior", "<f4"), ("albedo", "<f4", 3), ("pad", "<f4")])
QUAD_DTYPE = np.dtype([("Q", "<f4", 3), ("D", "<f4"), ("u", "<f4", 3), ("mat", "<i4"), ("v", "<f4", 3), ("pad0", "<f4"),
                       ("w", "<f4", 3), ("pad1", "<f4"), ("n", "<f4", 3), ("pad2", "<f4")])
INSTANCE_DTYPE = np.dtype([("sin_t", "<f4"), ("cos_t", "<f4"), ("offset", "<f4", 3), ("child", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
MEDIUM_DTYPE = np.dtype([("boundary", "<i4"), ("neg_inv_density", "<f4"), ("mat", "<i4"), ("pad", "<i4")])

# every symbol include/rt_abi.h declares
RT_ABI_SYMBOLS = ["rt_init", "rt_shutdown", "rt_strerror", "rt_last_hip_error", "rt_last_error_detail", "rt_scene_create",
                  "rt_scene_destroy", "rt_frame_local_rows", "rt_local_to_global_row", "rt_render", "rt_frame_finish",
                  "rt_set_option", "rt_reset_options", "rt_scene_walk_info", "rt_init_devices", "rt_multi_create", "rt_multi_render",
                  "rt_multi_destroy", "rt_multi_device_count", "rt_multi_row_owner", "rt_multi_probe_rccl", "rt_multi_debug_uninterleave",
                  "rt_progressive_state_create", "rt_progressive_state_destroy", "rt_render_window",
                  "rt_plan_walk_array", "rt_regroup_leaves", "rt_trace_rays", "rt_render_adaptive",
                  "rt_radiance_rays", "rt_render_aov", "rt_render_aov_through", "rt_denoise_workspace_bytes", "rt_denoise", "rt_render_variance",
                  "rt_denoise_variance", "rt_scene_set_camera", "rt_scene_get_camera", "rt_multi_set_camera", "rt_reproject",
                  "rt_reproject_matrix", "rt_debug_rank", "rt_debug_prior", "rt_debug_cal_cost", "rt_debug_rank_info",
                  "rt_scene_update_spheres", "rt_scene_get_spheres", "rt_multi_update_spheres", "rt_refit_nodes", "rt_debug_scene_boxes",
                  "rt_reproject_moving", "rt_debug_cost_map", "rt_debug_set_cost_map",
                  "rt_scene_update_instances", "rt_scene_get_instances", "rt_refit_instances", "rt_multi_update_instances",
                  "rt_debug_box_tests", "rt_reproject_instances",
                  "rt_scene_update_quads", "rt_scene_get_quads", "rt_refit_quads", "rt_multi_update_quads", "rt_debug_scene_quads",
                  "rt_reproject_quads", "rt_debug_arith_tests", "rt_debug_math_tests", "rt_upscale", "rt_debug_tier_room"]

_rt = None
_host = None


def build(verbose: bool = False) -> None:
    """Compile both libraries and the drop-in executable in-tree (hipcc --offload-arch=gfx950)."""
    r = subprocess.run(["make", "-C", PKG_DIR, "-j8", "all"], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:])
        print(r.stderr[-4000:])
    if r.returncode != 0:
        raise RtError("building the HIP render library failed")


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise RtError(f"{HOST_LIB_PATH} not built (run __graft_entry__.build())")
        L = C.CDLL(HOST_LIB_PATH)
        L.rtw_last_error.restype = C.c_char_p
        L.rtw_scene_name.restype = C.c_char_p
        L.rtw_scene_name.argtypes = [C.c_int]
        L.rtw_scene_build.restype = C.c_void_p
        L.rtw_scene_build.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.rtw_scene_free.argtypes = [C.c_void_p]
        L.rtw_scene_desc.restype = C.POINTER(RtSceneDesc)
        L.rtw_scene_desc.argtypes = [C.c_void_p]
        L.rtw_scene_defaults.restype = C.c_float
        L.rtw_scene_defaults.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.rtw_scene_leaf_order.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rtw_rotation.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.rtw_quad_record.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_void_p]
        L.rtw_box_records.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_void_p]
        L.rtw_write_ppm.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.rtw_load_ppm.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.rtw_camera_init.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float,
                                      C.c_double, C.c_double, C.POINTER(RtCamera)]
        _host = L
    return _host


def rt_lib():
    """The HIP render library.  Raises when it has not been built -- there is nothing to fall back to."""
    global _rt
    if _rt is None:
        if not os.path.exists(RT_LIB_PATH):
            raise RtError(f"{RT_LIB_PATH} not built (run __graft_entry__.build()); the render path has no CPU fallback")
        L = C.CDLL(RT_LIB_PATH)
        L.rt_init.argtypes = [C.c_int]
        L.rt_strerror.restype = C.c_char_p
        L.rt_strerror.argtypes = [C.c_int]
        L.rt_last_error_detail.restype = C.c_char_p
        L.rt_scene_create.argtypes = [C.POINTER(RtSceneDesc), C.POINTER(C.c_void_p)]
        L.rt_scene_destroy.argtypes = [C.c_void_p]
        L.rt_frame_local_rows.argtypes = [C.POINTER(RtFrameDesc)]
        L.rt_local_to_global_row.argtypes = [C.POINTER(RtFrameDesc), C.c_int32]
        L.rt_render.argtypes = [C.c_void_p, C.POINTER(RtFrameDesc), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(RtStats)]
        L.rt_frame_finish.argtypes = [C.c_void_p, C.POINTER(RtStats)]
        L.rt_set_option.argtypes = [C.c_char_p, C.c_int]
        L.rt_init_devices.argtypes = [C.c_int]
        L.rt_multi_create.argtypes = [C.POINTER(RtSceneDesc), C.c_int, C.POINTER(C.c_void_p)]
        L.rt_multi_render.argtypes = [C.c_void_p, C.POINTER(RtFrameDesc), C.c_void_p, C.c_int, C.c_int, C.POINTER(RtStats)]
        L.rt_multi_destroy.argtypes = [C.c_void_p]
        L.rt_multi_device_count.argtypes = [C.c_void_p]
        L.rt_multi_row_owner.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.rt_progressive_state_create.argtypes = [C.c_void_p, C.POINTER(RtFrameDesc), C.POINTER(C.c_void_p)]
        L.rt_progressive_state_destroy.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_render_window.argtypes = [C.c_void_p, C.POINTER(RtFrameDesc), C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int, C.POINTER(RtStats)]
        L.rt_multi_probe_rccl.argtypes = [C.c_char_p]
        L.rt_multi_debug_uninterleave.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.rt_plan_walk_array.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_int32, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.rt_regroup_leaves.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.rt_regroup_leaves.restype = C.c_int
        L.rt_trace_rays.argtypes = [C.c_void_p, C.POINTER(RtRayBatch), C.c_void_p, C.c_int]
        L.rt_radiance_rays.argtypes = [C.c_void_p, C.POINTER(RtRadianceBatch), C.c_void_p, C.c_int]
        L.rt_render_aov.argtypes = [C.c_void_p, C.POINTER(RtFrameDesc), C.POINTER(RtAovDesc), C.c_int, C.c_void_p, C.c_int]
        L.rt_render_aov_through.argtypes = [C.c_void_p, C.POINTER(RtFrameDesc), C.POINTER(RtAovDesc), C.POINTER(RtAovThroughDesc), C.c_int,
                                            C.c_void_p, C.c_int]
        L.rt_denoise_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
        L.rt_denoise_workspace_bytes.restype = C.c_size_t
        L.rt_denoise.argtypes = [C.POINTER(RtDenoiseDesc), C.c_int, C.c_void_p, C.c_int]
        L.rt_render_adaptive.argtypes = [C.c_void_p, C.POINTER(RtFrameDesc), C.POINTER(RtAdaptiveDesc), C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.POINTER(RtStats)]
        L.rt_render_variance.argtypes = [C.c_void_p, C.POINTER(RtFrameDesc), C.POINTER(RtVarianceDesc), C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.POINTER(RtStats)]
        L.rt_denoise_variance.argtypes = [C.POINTER(RtDenoiseDesc), C.POINTER(RtDenoiseVarianceDesc), C.c_int, C.c_void_p, C.c_int]
        if hasattr(L, "rt_upscale"):   # (absent from an older library measured through RT_LIB_OVERRIDE)
            L.rt_upscale.argtypes = [C.POINTER(RtUpscaleDesc), C.c_int, C.c_void_p, C.c_int]
        L.rt_scene_set_camera.argtypes = [C.c_void_p, C.POINTER(RtCamera), C.c_int]
        L.rt_scene_get_camera.argtypes = [C.c_void_p, C.POINTER(RtCamera)]
        L.rt_multi_set_camera.argtypes = [C.c_void_p, C.POINTER(RtCamera), C.c_int]
        L.rt_scene_update_spheres.argtypes = [C.c_void_p, C.POINTER(RtSphereUpdate), C.c_int, C.c_int, C.c_void_p]
        L.rt_scene_get_spheres.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.rt_multi_update_spheres.argtypes = [C.c_void_p, C.POINTER(RtSphereUpdate), C.c_int]
        L.rt_refit_nodes.argtypes = [C.POINTER(RtSceneDesc), C.POINTER(RtSphereUpdate), C.c_void_p, C.c_void_p]
        L.rt_scene_update_instances.argtypes = [C.c_void_p, C.POINTER(RtInstanceUpdate), C.c_int, C.c_int, C.c_void_p]
        L.rt_scene_get_instances.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.rt_multi_update_instances.argtypes = [C.c_void_p, C.POINTER(RtInstanceUpdate), C.c_int]
        L.rt_refit_instances.argtypes = [C.POINTER(RtSceneDesc), C.POINTER(RtInstanceUpdate), C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_scene_update_quads"):   # (absent from an older library measured through RT_LIB_OVERRIDE)
            L.rt_scene_update_quads.argtypes = [C.c_void_p, C.POINTER(RtQuadUpdate), C.c_int, C.c_int, C.c_void_p]
            L.rt_scene_get_quads.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
            L.rt_multi_update_quads.argtypes = [C.c_void_p, C.POINTER(RtQuadUpdate), C.c_int]
            L.rt_refit_quads.argtypes = [C.POINTER(RtSceneDesc), C.POINTER(RtQuadUpdate), C.c_void_p, C.c_void_p]
            L.rt_debug_scene_quads.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.rt_debug_scene_boxes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.rt_reproject.argtypes = [C.POINTER(RtReprojectDesc), C.c_int, C.c_void_p, C.c_int]
        L.rt_reproject_matrix.argtypes = [C.POINTER(RtCamera), C.POINTER(C.c_float)]
        L.rt_reproject_moving.argtypes = [C.POINTER(RtReprojectDesc), C.POINTER(RtReprojectMotionDesc), C.c_int, C.c_void_p, C.c_int]
        if hasattr(L, "rt_reproject_instances"):   # (absent from an older library measured through RT_LIB_OVERRIDE)
            L.rt_reproject_instances.argtypes = [C.POINTER(RtReprojectDesc), C.POINTER(RtReprojectMotionDesc), C.POINTER(RtReprojectInstanceDesc),
                                                 C.c_int, C.c_void_p, C.c_int]
        if hasattr(L, "rt_reproject_quads"):
            L.rt_reproject_quads.argtypes = [C.POINTER(RtReprojectDesc), C.POINTER(RtReprojectMotionDesc), C.POINTER(RtReprojectInstanceDesc),
                                             C.POINTER(RtReprojectQuadDesc), C.c_int, C.c_void_p, C.c_int]
        L.rt_debug_adaptive_passes.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.rt_debug_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_debug_prior.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_uint64)]
        L.rt_debug_cal_cost.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.rt_debug_rank_info.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_debug_cost_map"):   # (absent from an older library measured through RT_LIB_OVERRIDE)
            L.rt_debug_cost_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
            L.rt_debug_set_cost_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        if hasattr(L, "rt_debug_box_tests"):   # (likewise)
            L.rt_debug_box_tests.argtypes = [C.c_int32] + [C.c_void_p] * 8
        if hasattr(L, "rt_debug_arith_tests"):   # (likewise)
            L.rt_debug_arith_tests.argtypes = [C.c_int32, C.c_int64] + [C.c_void_p] * 5
        if hasattr(L, "rt_debug_math_tests"):   # (likewise)
            L.rt_debug_math_tests.argtypes = [C.c_int32, C.c_int32, C.c_uint32, C.c_int64, C.c_float] + [C.c_void_p] * 5
        L.rt_scene_walk_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        if hasattr(L, "rt_debug_tier_room"):   # (absent from an older library measured through RT_LIB_OVERRIDE)
            L.rt_debug_tier_room.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        _rt = L
    return _rt


def _check(st: int, what: str) -> None:
    if st != 0:
        L = rt_lib()
        raise RtError(f"{what}: {L.rt_strerror(st).decode()} -- {L.rt_last_error_detail().decode()}")


def _status(st: int, entry: str) -> None:
    """_check for the entries that refuse their arguments: RT_ERR_INVALID is a ValueError that carries the library's detail."""
    if st == 1:
        raise ValueError(rt_lib().rt_last_error_detail().decode())
    _check(st, entry)


def _stream_arg(stream):
    """What the C entries take as a stream: 0 / None (the null stream), a hipStream_t as an integer or a torch.cuda.Stream."""
    if hasattr(stream, "cuda_stream"):
        stream = stream.cuda_stream
    return C.c_void_p(int(stream)) if stream else None


def _enqueue_on(dev, stream, tensors):
    """The torch stream a call that touches `tensors` is launched on: `stream`, or the current stream of `dev` for None.
    Without tensors (a call that launches nothing) there is nothing to hand over."""
    import torch
    current = torch.cuda.current_stream(dev)
    if stream is None:
        return current
    if stream == current or not tensors:
        return stream
    # The inputs' contiguous copies and the outputs were made on the current stream: `stream` waits for that
    # work (and for whatever last used the outputs' blocks there) before the call writes, and the caching
    # allocator must not hand any of them out again before `stream` is done with them.
    stream.wait_stream(current)
    for x in tensors:
        if x is not None:
            x.record_stream(stream)
    return stream


_TORCH_DTYPE_NAMES = {}   # torch.float32 -> "float32", filled as dtypes are met (str() of one is slow)


class _Buffers:
    """The one rule for the buffers of a call.  Built once per call from its anchor argument `name`: whether that is a numpy
    array decides whether the call is a host call (numpy arrays) or a device call (torch tensors on cuda:`device`, or the
    device of init() for None), and every other buffer must be of the anchor's kind.  Each refusal is a ValueError that
    starts with the argument's name; no check allocates or copies anything."""
    __slots__ = ("on_host", "anchor", "device", "dev")

    def __init__(self, on_host, name, device):
        self.on_host, self.anchor, self.device, self.dev = on_host, name, device, None

    def torch_device(self):
        """The torch device of a device call (torch is imported only when a tensor is looked at or made)."""
        if self.dev is None:
            import torch
            self.dev = torch.device("cuda", 0 if self.device is None else self.device)
        return self.dev

    def wrong_kind(self, name, array, pointer=False):
        """The refusal of an argument that is no buffer of the call's kind (the anchor itself may be of either)."""
        kinds = [array] if self.on_host or name == self.anchor else []
        if not self.on_host:
            kinds += ["a torch tensor", "an integer device pointer"] if pointer else ["a torch tensor"]
        return ValueError(f"{name}: {' or '.join(kinds)} is expected" + ("" if name == self.anchor else f" ({self.anchor} is one)"))

    def address(self, x, name, dtypes=("float32",), shape=None, count=None, strided=False, pointer=False):
        """The address of x checked: None, or an array / tensor of one of `dtypes` (names; None: any) with exactly `shape` or
        `count` elements, contiguous unless `strided` -- or, in a device call with `pointer`, device memory as an integer."""
        if x is None:
            return None
        on_host = self.on_host
        if on_host:
            if not isinstance(x, np.ndarray):
                raise self.wrong_kind(name, "a numpy array")
            dtype, contiguous = x.dtype.name, x.flags["C_CONTIGUOUS"]
        elif hasattr(x, "data_ptr"):
            if x.device != (self.dev or self.torch_device()):
                raise ValueError(f"{name}: tensor on {x.device}, expected on {self.dev}")
            dtype = _TORCH_DTYPE_NAMES.get(x.dtype) or _TORCH_DTYPE_NAMES.setdefault(x.dtype, str(x.dtype)[6:])
            contiguous = x.is_contiguous()
        elif pointer and isinstance(x, (int, np.integer)) and not isinstance(x, bool):
            return int(x)
        else:
            raise self.wrong_kind(name, "a numpy array", pointer)
        if dtypes is not None and dtype not in dtypes:
            raise ValueError(f"{name}: {' or '.join(dtypes)} expected, got {dtype}")
        if shape is not None and x.shape != shape:
            raise ValueError(f"{name}: shape {tuple(x.shape)}, expected {shape}")
        if count is not None and (x.size if on_host else x.numel()) != count:
            raise ValueError(f"{name}: shape {tuple(x.shape)}, expected {count} elements")
        if not (strided or contiguous):
            raise ValueError(f"{name}: a {'C-contiguous array' if on_host else 'contiguous tensor'} is expected")
        return x.ctypes.data if on_host else x.data_ptr()

    def empty(self, shape, dtype="float32"):
        """A new buffer of the anchor's kind: a numpy array, or a tensor on the device."""
        if self.on_host:
            return np.empty(shape, dtype)
        import torch
        return torch.empty(shape, dtype=getattr(torch, dtype), device=self.torch_device())

    def table(self, x, name, dtype, dtype_name):
        """A table of records: a one-dimensional numpy array of `dtype` (made contiguous), or in a device call a contiguous
        (n, dtype.itemsize // 4) tensor of a 4-byte dtype, read in place.  Returns (count, its address or None without a
        record, what must stay referenced until the C call has returned): the caller stores the third on something that
        outlives the call -- here as an attribute of the ctypes structure that holds the address, which a Structure
        instance allows beside its fields and which lives as long as the structure does."""
        words = dtype.itemsize // 4
        if self.on_host:
            if not isinstance(x, np.ndarray) or x.dtype != dtype or x.ndim != 1:
                raise self.wrong_kind(name, f"a one-dimensional numpy array of {dtype_name}")
            x = np.ascontiguousarray(x)
            return len(x), (x.ctypes.data if len(x) else None), x
        if not hasattr(x, "data_ptr"):
            raise self.wrong_kind(name, f"a one-dimensional numpy array of {dtype_name}")
        if x.device != self.torch_device():
            raise ValueError(f"{name}: tensor on {x.device}, expected on {self.dev}")
        if x.ndim != 2 or x.shape[1] != words or x.element_size() != 4:
            raise ValueError(f"{name}: shape {tuple(x.shape)} of {x.dtype}, expected (n, {words}) of a 4-byte dtype")
        if not x.is_contiguous():
            raise ValueError(f"{name}: a contiguous tensor is expected (it is read in place)")
        return int(x.shape[0]), (x.data_ptr() if x.shape[0] else None), x


def load_ppm(path: str):
    """Texture pixels from a PPM file -> (uint8 array h*w*3, w, h)."""
    L = host_lib()
    w, h = C.c_int(0), C.c_int(0)
    n = L.rtw_load_ppm(path.encode(), None, 0, C.byref(w), C.byref(h))
    if n < 0:
        raise RtError(f"cannot read PPM {path}")
    buf = np.zeros(n, np.uint8)
    L.rtw_load_ppm(path.encode(), buf.ctypes.data, n, C.byref(w), C.byref(h))
    return buf, w.value, h.value


SCENE_TEXTURES = {"earth": "earthmap.ppm", "final": "earthmap.ppm", "simple_light": "poolball.ppm", "original": "8ball.ppm",
                  "instanced": "earthmap.ppm"}


def default_texture(scene: str = "final"):
    """The image a reference scene loads (main.cu:816,1010,1186,1254), decoded once to assets/*.ppm; (None,0,0) otherwise."""
    name = SCENE_TEXTURES.get(scene)
    if name is None:
        return None, 0, 0
    p = os.path.join(REPO_ROOT, "assets", name)
    return load_ppm(p) if os.path.exists(p) else (None, 0, 0)


class HostScene:
    """A reference scene built and flattened on the host (no GPU involved)."""

    def __init__(self, name: str, nx: int = 0, ny: int = 0, image=None, iw: int = 0, ih: int = 0):
        L = host_lib()
        self._image = None if image is None else np.ascontiguousarray(image, np.uint8)
        ptr = None if self._image is None else self._image.ctypes.data
        self._h = L.rtw_scene_build(name.encode(), nx, ny, ptr, iw, ih)
        if not self._h:
            raise RtError(f"scene '{name}': {L.rtw_last_error().decode()}")
        self.name = name
        self.desc = L.rtw_scene_desc(self._h).contents
        out4 = (C.c_int * 4)()
        bg = (C.c_float * 3)()
        dbl = C.c_int(0)
        self.gamma = float(L.rtw_scene_defaults(self._h, out4, bg, C.byref(dbl)))
        self.nx, self.ny, self.ns, self.use_gradient_bg = (int(x) for x in out4)
        self.background = [float(x) for x in bg]
        self.ppm_double_scale = bool(dbl.value)

    def nodes(self) -> np.ndarray:
        n = self.desc.n_nodes
        buf = (C.c_char * (n * NODE_DTYPE.itemsize)).from_address(self.desc.nodes)
        return np.frombuffer(buf, NODE_DTYPE, n).copy()

    def spheres(self) -> np.ndarray:
        n = self.desc.n_spheres
        buf = (C.c_char * (n * SPHERE_DTYPE.itemsize)).from_address(self.desc.spheres)
        return np.frombuffer(buf, SPHERE_DTYPE, n).copy()

    def materials(self) -> np.ndarray:
        n = self.desc.n_materials
        buf = (C.c_char * (n * MATERIAL_DTYPE.itemsize)).from_address(self.desc.materials)
        return np.frombuffer(buf, MATERIAL_DTYPE, n).copy()

    def _array(self, ptr, n, dtype) -> np.ndarray:
        if n == 0:
            return np.zeros(0, dtype)
        buf = (C.c_char * (n * dtype.itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype, n).copy()

    def quads(self) -> np.ndarray:
        return self._array(self.desc.quads, self.desc.n_quads, QUAD_DTYPE)

    def instances(self) -> np.ndarray:
        return self._array(self.desc.instances, self.desc.n_instances, INSTANCE_DTYPE)

    def media(self) -> np.ndarray:
        return self._array(self.desc.media, self.desc.n_media, MEDIUM_DTYPE)

    def leaf_order(self) -> np.ndarray:
        L = host_lib()
        n = self.desc.n_nodes
        out = np.zeros(n, np.int32)
        L.rtw_scene_leaf_order(self._h, out.ctypes.data, n)
        return out

    def frame(self, nx=None, ny=None, ns=None, gamma=None, seed_base=1984, tile_rows=None, tile_first=0, tile_stride=1) -> RtFrameDesc:
        f = RtFrameDesc()
        f.nx = self.nx if nx is None else nx
        f.ny = self.ny if ny is None else ny
        f.ns = self.ns if ns is None else ns
        f.gamma = self.gamma if gamma is None else gamma
        f.background[:] = self.background
        f.use_gradient_bg = self.use_gradient_bg
        f.seed_base = seed_base
        f.tile_rows = f.ny if tile_rows is None else tile_rows
        f.tile_first = tile_first
        f.tile_stride = tile_stride
        return f

    def close(self):
        if getattr(self, "_h", None):
            host_lib().rtw_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _frame_buffers(color):
    """The buffer rule of denoise() and reproject(), whose anchor is the frame `color` (ny, nx, 3) on the device of init(), and (nx, ny)."""
    bufs = _Buffers(isinstance(color, np.ndarray), "color", _initialised_device)
    if not (bufs.on_host or hasattr(color, "data_ptr")):
        raise bufs.wrong_kind("color", "a numpy array")
    if color.ndim != 3 or color.shape[2] != 3 or color.shape[0] < 1 or color.shape[1] < 1:
        raise ValueError(f"color: shape {tuple(color.shape)}, expected (ny, nx, 3)")
    ny, nx = int(color.shape[0]), int(color.shape[1])
    if nx * ny >= 1 << 31:
        raise ValueError("frame too large")
    return bufs, nx, ny


_initialised_device = None


def init(device: int = 0) -> None:
    global _initialised_device
    _check(rt_lib().rt_init(device), "rt_init")
    _initialised_device = device


def set_option(key: str, value: int) -> None:
    _check(rt_lib().rt_set_option(key.encode(), int(value)), f"rt_set_option({key})")


def reset_options() -> None:
    """Every scheduling knob back to the shipped default."""
    _check(rt_lib().rt_reset_options(), "rt_reset_options")


# ---- the order of the tail hand-off queue (csrc/rt_handoff_order.h), restated in NumPy
HANDOFF_SUB_BITS = 2
HANDOFF_BUCKETS = 1 + 64 * (1 << HANDOFF_SUB_BITS)
HANDOFF_ORDER_MIN_PER_WAVE, HANDOFF_ORDER_MAX_PER_WAVE = 2, 32


def handoff_order_key(entries, costs, sample_begin: int, sample_end: int):
    """Remaining-work key of hand-off queue entries (next sample << 32 | pixel) whose pixels' parked costs are `costs`, entry for
    entry: (sample_end - next) * (rays so far + 1) // (samples done + 1), exact, as an object array of Python integers."""
    e = np.asarray(entries, np.uint64)
    nxt = (e >> np.uint64(32)).astype(np.int64)
    rays = (np.asarray(costs, np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)
    to_go, done = np.maximum(int(sample_end) - nxt, 0), np.maximum(nxt - int(sample_begin), 0)
    return np.array([int(t) * (int(r) + 1) // (int(d) + 1) for t, r, d in zip(to_go, rays, done)], dtype=object)


def handoff_order_bucket(keys):
    """Bucket of each key on the fixed logarithmic scale: 0 for key 0, else 1 + 4 e + m with e the key's leading bit and m the two
    bits below it (zeros shifted in under e < 2).  The ordered queue holds its entries in non-increasing bucket order."""
    out = np.zeros(len(keys), np.int64)
    for i, k in enumerate(keys):
        k = int(k)
        if k > 0:
            e = k.bit_length() - 1
            m = (k >> (e - HANDOFF_SUB_BITS) if e >= HANDOFF_SUB_BITS else k << (HANDOFF_SUB_BITS - e)) & ((1 << HANDOFF_SUB_BITS) - 1)
            out[i] = 1 + (e << HANDOFF_SUB_BITS) + m
    return out


def debug_order_handoff(entries, costs, sample_begin: int, sample_end: int, tail_waves: int):
    """rt_debug_order_handoff (tests): the ordering launch of one tail on n entries (every pixel below n; costs[pixel] its parked
    cost) for a tail launch of `tail_waves` waves.  Returns (the ordered queue, spare slots behind it that were written)."""
    e, c = np.ascontiguousarray(entries, np.uint64), np.ascontiguousarray(costs, np.uint32)
    assert e.ndim == 1 and c.shape == e.shape
    out, overrun = np.zeros(len(e), np.uint64), C.c_uint32(0xFFFFFFFF)
    L = rt_lib()
    L.rt_debug_order_handoff.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_uint32)]
    _check(L.rt_debug_order_handoff(e.ctypes.data if len(e) else None, c.ctypes.data if len(e) else None, len(e), int(sample_begin), int(sample_end),
                                    int(tail_waves), out.ctypes.data if len(e) else None, C.byref(overrun)), "rt_debug_order_handoff")
    return out, int(overrun.value)


def denoise_workspace_bytes(nx: int, ny: int) -> int:
    """Bytes of device memory rt_denoise wants as its workspace for an nx x ny frame (0 for a bad size)."""
    return int(rt_lib().rt_denoise_workspace_bytes(int(nx), int(ny)))


def denoise(color, albedo=None, normal=None, depth=None, *, iterations=DENOISE_DEFAULTS["iterations"],
            sigma_color=None, color_floor=DENOISE_DEFAULTS["color_floor"],
            normal_sharpness=DENOISE_DEFAULTS["normal_sharpness"], sigma_depth=DENOISE_DEFAULTS["sigma_depth"], demodulate=None,
            out=None, workspace=None, stream=0, blocking=True, variance=None, variance_out=None,
            sigma_variance=DENOISE_VARIANCE_DEFAULTS["sigma_variance"], variance_floor=DENOISE_VARIANCE_DEFAULTS["variance_floor"]):
    """The edge-avoiding a-trous filter of rt_denoise (include/rt_abi.h): a noisy linear frame `color` (ny, nx, 3), guided by
    the feature buffers of render_aov -- albedo, normal (ny, nx, 3) and depth (ny, nx), each optional.  It runs on the device
    of init().

    Either all numpy float32 arrays (C-contiguous; the call waits; `workspace` must be None) or all contiguous float32
    torch tensors on that device: zero-copy, enqueued on `stream` (a hipStream_t as an integer or a torch.cuda.Stream) and
    waited for only with blocking=True.  out: None (an array or tensor like color is made) or one of the same kind and
    shape; it may be `color` itself (in place).  workspace: None (the library allocates its own and the call waits) or a
    contiguous torch tensor of at least denoise_workspace_bytes(nx, ny) bytes on the device.  demodulate=None means "when
    albedo is given".  Returns out.  Malformed arguments raise ValueError before anything is launched.

    variance: None, or the per-pixel variance (ny, nx) that render_variance returns -- the filter then runs variance-guided
    (rt_denoise_variance): a tap is weighed by the squared colour difference over sigma_variance^2 times the two pixels'
    variances plus variance_floor, in place of the colour factor, so sigma_color is passed as 0 and an explicit non-zero
    one is a ValueError.  variance_out: None or an array / tensor (ny, nx) that receives the filtered variance.  sigma_color=None
    means DENOISE_DEFAULTS["sigma_color"] without a variance."""
    if variance is None:
        if variance_out is not None:
            raise ValueError("variance_out needs variance")
        if sigma_color is None:
            sigma_color = DENOISE_DEFAULTS["sigma_color"]
    else:
        if sigma_color is not None and float(sigma_color) != 0:
            raise ValueError("sigma_color must be left out or 0 with a variance: the variance factor replaces the colour factor")
        sigma_color = 0.0
        sigma_variance, variance_floor = float(sigma_variance), float(variance_floor)
        if not (np.isfinite(sigma_variance) and np.float32(1e-6) <= np.float32(sigma_variance) <= np.float32(1e6)):
            raise ValueError("sigma_variance must be in [1e-6, 1e6]")
        if not (np.isfinite(variance_floor) and 0 < np.float32(variance_floor) < np.inf):
            raise ValueError("variance_floor must be finite and positive")
    bufs, nx, ny = _frame_buffers(color)
    for k, v, lo, hi in (("iterations", iterations, 1, 8), ("normal_sharpness", normal_sharpness, 0, 10)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{k} must be an integer in {lo}..{hi}")
    sigma_color, color_floor, sigma_depth = float(sigma_color), float(color_floor), float(sigma_depth)
    for k, v in (("sigma_color", sigma_color), ("sigma_depth", sigma_depth)):
        if not (v == 0 or (np.isfinite(v) and np.float32(1e-6) <= np.float32(v) <= np.float32(1e6))):
            raise ValueError(f"{k} must be 0 or in [1e-6, 1e6]")
    if sigma_color > 0 and not (np.isfinite(color_floor) and 0 < np.float32(color_floor) < np.inf):
        raise ValueError("color_floor must be finite and positive")
    if demodulate is None:
        demodulate = albedo is not None
    if demodulate and albedo is None:
        raise ValueError("demodulate needs albedo")
    if bufs.on_host and workspace is not None:
        raise ValueError("workspace: device memory goes with device tensors; pass None with numpy arrays")
    rgb, one = (ny, nx, 3), (ny, nx)
    d = RtDenoiseDesc()
    d.nx, d.ny = nx, ny
    d.color, d.albedo, d.normal = (bufs.address(x, k, shape=rgb) for k, x in (("color", color), ("albedo", albedo), ("normal", normal)))
    d.depth, d.out = bufs.address(depth, "depth", shape=one), bufs.address(out, "out", shape=rgb)
    if workspace is not None:
        d.workspace = bufs.address(workspace, "workspace", None)
        d.workspace_bytes = workspace.numel() * workspace.element_size()
    d.iterations, d.normal_sharpness, d.demodulate = int(iterations), int(normal_sharpness), 1 if demodulate else 0
    d.sigma_color, d.color_floor, d.sigma_depth = sigma_color, color_floor, sigma_depth
    args = (0 if bufs.on_host else 1, _stream_arg(stream), 1 if blocking else 0)
    if variance is not None:
        vd = RtDenoiseVarianceDesc()
        vd.variance, vd.variance_out = bufs.address(variance, "variance", shape=one), bufs.address(variance_out, "variance_out", shape=one)
        vd.sigma_variance, vd.variance_floor = sigma_variance, variance_floor
    if out is None:   # (made last: every check has passed)
        out = bufs.empty(rgb)
        d.out = bufs.address(out, "out", shape=rgb)
    L = rt_lib()
    if variance is None:
        st = L.rt_denoise(C.byref(d), *args)
    else:
        st = L.rt_denoise_variance(C.byref(d), C.byref(vd), *args)
    _status(st, "rt_denoise" if variance is None else "rt_denoise_variance")
    return out


def upscale(color_lo, factor, albedo_lo=None, normal_lo=None, depth_lo=None, albedo=None, normal=None, depth=None, *,
            normal_sharpness=UPSCALE_DEFAULTS["normal_sharpness"], sigma_depth=UPSCALE_DEFAULTS["sigma_depth"],
            min_weight=UPSCALE_DEFAULTS["min_weight"], demodulate=None, out=None, weight_out=None, stream=0, blocking=True):
    """The guided upscaler of rt_upscale (include/rt_abi.h): a coarse linear frame `color_lo` (ly, lx, 3) -- render() at gamma 1
    of the nx/factor x ny/factor frame of a camera -- rebuilt at `factor` times the size, guided by the feature buffers of
    render_aov on both grids: albedo_lo, normal_lo (ly, lx, 3) and depth_lo (ly, lx) of the coarse frame, albedo, normal
    (ny, nx, 3) and depth (ny, nx) of the full one, each optional; a normal or a depth takes part only when given on both
    grids, and one given on one grid only is a ValueError.  It runs on the device of init().

    Either all numpy float32 arrays (C-contiguous; the call waits) or all contiguous float32 torch tensors on that device:
    zero-copy, enqueued on `stream` (a hipStream_t as an integer or a torch.cuda.Stream) and waited for only with
    blocking=True.  The output is (factor ly, factor lx, 3); a full-resolution guide must have that size.  out: None (an
    array or tensor is made) or one of that shape; weight_out: None or (ny, nx), receives W / W0, the share of the spline's
    weight the guides let through.  demodulate=None means "when both albedos are given".  Returns out.  Malformed arguments
    raise ValueError before anything is launched."""
    bufs = _Buffers(isinstance(color_lo, np.ndarray), "color_lo", _initialised_device)
    if not (bufs.on_host or hasattr(color_lo, "data_ptr")):
        raise bufs.wrong_kind("color_lo", "a numpy array")
    if color_lo.ndim != 3 or color_lo.shape[2] != 3 or color_lo.shape[0] < 1 or color_lo.shape[1] < 1:
        raise ValueError(f"color_lo: shape {tuple(color_lo.shape)}, expected (ly, lx, 3)")
    if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or not 2 <= int(factor) <= 8:
        raise ValueError("factor must be an integer in 2..8")
    if isinstance(normal_sharpness, bool) or not isinstance(normal_sharpness, (int, np.integer)) or not 0 <= int(normal_sharpness) <= 10:
        raise ValueError("normal_sharpness must be an integer in 0..10")
    sigma_depth, min_weight = float(sigma_depth), float(min_weight)
    if not (sigma_depth == 0 or (np.isfinite(sigma_depth) and np.float32(1e-6) <= np.float32(sigma_depth) <= np.float32(1e6))):
        raise ValueError("sigma_depth must be 0 or in [1e-6, 1e6]")
    if not (np.isfinite(min_weight) and 0 <= min_weight <= 1):
        raise ValueError("min_weight must be in [0, 1]")
    factor, ly, lx = int(factor), int(color_lo.shape[0]), int(color_lo.shape[1])
    ny, nx = factor * ly, factor * lx
    if nx * ny >= 1 << 31:
        raise ValueError("frame too large")
    for k, v in (("albedo", albedo), ("normal", normal), ("depth", depth)):
        if v is not None and hasattr(v, "shape") and tuple(v.shape[:2]) != (ny, nx):
            raise ValueError(f"{k}: shape {tuple(v.shape)}, but factor {factor} times the coarse frame is {ny} x {nx}")
    for k, a, b in (("normal", normal, normal_lo), ("depth", depth, depth_lo)):
        if (a is None) != (b is None):
            raise ValueError(f"{k} and {k}_lo must both be given or both be left out")
    if demodulate is None:
        demodulate = albedo_lo is not None and albedo is not None
    if demodulate and (albedo_lo is None or albedo is None):
        raise ValueError("demodulate needs albedo_lo and albedo")
    rgb_lo, one_lo, rgb, one = (ly, lx, 3), (ly, lx), (ny, nx, 3), (ny, nx)
    d = RtUpscaleDesc()
    d.nx, d.ny, d.factor, d.normal_sharpness, d.demodulate = nx, ny, factor, int(normal_sharpness), 1 if demodulate else 0
    d.sigma_depth, d.min_weight = sigma_depth, min_weight
    d.color_lo, d.albedo_lo, d.normal_lo = (bufs.address(x, k, shape=rgb_lo) for k, x in (("color_lo", color_lo), ("albedo_lo", albedo_lo), ("normal_lo", normal_lo)))
    d.depth_lo = bufs.address(depth_lo, "depth_lo", shape=one_lo)
    d.albedo, d.normal, d.depth = bufs.address(albedo, "albedo", shape=rgb), bufs.address(normal, "normal", shape=rgb), bufs.address(depth, "depth", shape=one)
    d.out, d.weight_out = bufs.address(out, "out", shape=rgb), bufs.address(weight_out, "weight_out", shape=one)
    if out is None:   # (made last: every check has passed)
        out = bufs.empty(rgb)
        d.out = bufs.address(out, "out", shape=rgb)
    _status(rt_lib().rt_upscale(C.byref(d), 0 if bufs.on_host else 1, _stream_arg(stream), 1 if blocking else 0), "rt_upscale")
    return out


_denoise = denoise   # (DeviceScene.render_upscaled has a parameter of that name)


def make_camera(lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist, t0=0.0, t1=0.0) -> RtCamera:
    """The rt_camera a reference scene function would construct from these arguments (camera.cuh:59-78): the host scene
    library's camera class, i.e. the reference's own float arithmetic -- what HostScene(name).desc.camera holds for the
    arguments in host/rtw_scenes.cpp.  lookfrom, lookat, vup: three floats each; vfov in degrees; [t0, t1]: the shutter."""
    v = [np.asarray(x, np.float64).reshape(-1) for x in (lookfrom, lookat, vup)]
    if any(len(x) != 3 for x in v):
        raise ValueError("lookfrom, lookat and vup: three floats each are expected")
    scalars = [float(x) for x in (vfov, aspect, aperture, focus_dist, t0, t1)]
    if not all(np.isfinite(x).all() for x in v) or not np.isfinite(scalars).all():
        raise ValueError("the camera arguments must be finite")
    if scalars[5] < scalars[4]:
        raise ValueError("t1 must not be before t0")
    a = [(C.c_float * 3)(*x) for x in v]
    c = RtCamera()
    if host_lib().rtw_camera_init(a[0], a[1], a[2], *scalars, C.byref(c)) != 0:
        raise RtError("rtw_camera_init failed")
    return c


def reproject_matrix(prev: RtCamera) -> np.ndarray:
    """rt_reproject_matrix: the 3 x 3 float32 matrix that takes a vector from `prev`'s origin to (a, a s, a t), its ray
    parameter and frame coordinates in `prev` (include/rt_abi.h).  Host only.  A singular camera is ValueError."""
    m = (C.c_float * 9)()
    _status(rt_lib().rt_reproject_matrix(C.byref(prev), m), "rt_reproject_matrix")
    return np.array(m, np.float32).reshape(3, 3)


def reproject(color, depth, alpha, cur: RtCamera, prev: RtCamera, normal=None, prim=None, history=None, history_len=None,
              prev_depth=None, prev_alpha=None, prev_normal=None, prev_prim=None, *, out=None, out_len=None, motion=False,
              alpha_min=REPROJECT_DEFAULTS["alpha_min"], depth_tol=REPROJECT_DEFAULTS["depth_tol"],
              normal_min=REPROJECT_DEFAULTS["normal_min"], max_history=REPROJECT_DEFAULTS["max_history"], stream=0, blocking=True,
              spheres=None, prev_spheres=None, media=None, time=None, prev_time=None,
              inst=None, prev_inst=None, instances=None, prev_instances=None, quads=None, prev_quads=None):
    """Temporal reprojection (rt_reproject, include/rt_abi.h): the current linear frame `color` (ny, nx, 3) blended into the
    history of the previous frame, fetched where each pixel's surface point -- from `depth` and `alpha` (ny, nx) of
    render_aov and the cameras `cur` and `prev` -- was in that frame.  history (ny, nx, 3) and history_len (ny, nx) are the
    previous call's out and length, prev_depth / prev_alpha the previous frame's depth and alpha; history=None is the first
    frame (out = color, length 1).  normal (ny, nx, 3) with prev_normal, and prim (ny, nx) int32 with prev_prim, switch on
    the normal and the id test of a tap.  It runs on the device of init().

    Either all numpy arrays (C-contiguous; the call waits) or all contiguous torch tensors on that device: zero-copy,
    enqueued on `stream` (a hipStream_t as an integer or a torch.cuda.Stream) and waited for only with blocking=True.  out /
    out_len: None (made like color) or arrays / tensors of the same kind; they may overlap no input.  motion: False, True (a
    (ny, nx, 2) buffer is made) or such a buffer.  Returns a ReprojectResult (out, length, motion).  Malformed arguments raise
    ValueError before anything is launched.

    spheres / prev_spheres (rt_reproject_moving): the sphere records the current and the previous frame were rendered with
    (DeviceScene.spheres() after and before update_spheres).  A surface pixel on a sphere whose record differs -- or in a
    medium bounded by one; `media` is the scene's media() -- is first carried back to where that surface point was, so the
    history follows the sphere and `motion` holds its motion too.  prim and prev_prim are then required.  With numpy buffers
    the tables are arrays of SPHERE_DTYPE / MEDIUM_DTYPE; with tensors they are contiguous (n, 8) / (n, 4) tensors of a
    4-byte dtype on the device, as update_spheres takes them.  time / prev_time: the instants at which centres c0 + t vel
    are taken; default: the shutter centre of `cur` / `prev`.  With spheres=None and instances=None the other four must be None too.

    instances / prev_instances (rt_reproject_instances): the instance records the current and the previous frame were rendered
    with (DeviceScene.instances() after and before update_instances), arrays of INSTANCE_DTYPE or (n, 8) tensors.  A surface
    pixel on an instance whose record differs -- or in a medium bounded by one -- is carried back through the two records, its
    normal with it.  inst (ny, nx) int32, render_aov's `inst` of the current frame, is then required beside prim and prev_prim,
    and prev_inst exactly when history is given; a tap must show the pixel's instance.  The sphere arguments stay optional
    beside these.  With instances=None and quads=None the other three must be None too.

    quads / prev_quads (rt_reproject_quads): the quad records the current and the previous frame were rendered with
    (DeviceScene.quads() after and before update_quads), arrays of QUAD_DTYPE or (n, 20) tensors.  A surface pixel on a quad --
    a face of a box is one -- whose Q, u or v differ is carried back through its planar coordinates, in the object space of
    its instance when it has one, and its normal becomes the previous record's.  inst is required (and prev_inst exactly when
    history is given) beside prim and prev_prim; instances / prev_instances and the sphere arguments stay optional beside
    these, with no record when absent -- but a quad under an instance is followed only with that instance's records given."""
    bufs, nx, ny = _frame_buffers(color)
    alpha_min, depth_tol, normal_min, max_history = (float(np.float32(x)) for x in (alpha_min, depth_tol, normal_min, max_history))
    if not 0 < alpha_min <= 1:
        raise ValueError("alpha_min must be in (0, 1]")
    if not 0 <= depth_tol <= 1:
        raise ValueError("depth_tol must be in [0, 1]")
    if not -1 <= normal_min <= 1:
        raise ValueError("normal_min must be in [-1, 1]")
    if not 1 <= max_history <= 65536:
        raise ValueError("max_history must be in [1, 65536]")
    if not isinstance(cur, RtCamera) or not isinstance(prev, RtCamera):
        raise ValueError("cur and prev: RtCamera structures are expected")
    if depth is None or alpha is None:
        raise ValueError("depth and alpha are required")
    if history is None:
        if any(x is not None for x in (history_len, prev_depth, prev_alpha)):
            raise ValueError("history_len, prev_depth and prev_alpha need history")
    elif any(x is None for x in (history_len, prev_depth, prev_alpha)):
        raise ValueError("history needs history_len, prev_depth and prev_alpha")
    md, imd, qmd = None, None, None
    if quads is None and prev_quads is not None:
        raise ValueError("prev_quads needs quads")
    if instances is None and quads is None and any(x is not None for x in (inst, prev_inst, prev_instances)):
        raise ValueError("inst, prev_inst and prev_instances need instances")
    if instances is None and prev_instances is not None:
        raise ValueError("prev_instances needs instances")
    if spheres is None and instances is None and quads is None:
        if any(x is not None for x in (prev_spheres, media, time, prev_time)):
            raise ValueError("prev_spheres, media, time and prev_time need spheres or instances")
    else:
        if spheres is None and prev_spheres is not None:
            raise ValueError("prev_spheres needs spheres")
        if spheres is not None and prev_spheres is None:
            raise ValueError("spheres needs prev_spheres")
        if prim is None or prev_prim is None:
            raise ValueError("spheres / instances: prim and prev_prim are required to follow what moved")
        def table_pair(name, current, previous, dtype, dtype_name):
            """The record tables of both frames: one dtype, equal lengths.  -> (count, address, what keeps it alive, the previous
            table's address, what keeps that alive); each structure keeps what its pointers point to, so that a numpy table is
            referenced until the C call has returned."""
            n, address, keep = bufs.table(current, name, dtype, dtype_name)
            n_prev, prev_address, prev_keep = bufs.table(previous, "prev_" + name, dtype, dtype_name)
            if n_prev != n:
                raise ValueError(f"prev_{name}: {n_prev} records, {name} has {n}")
            return n, address, keep, prev_address, prev_keep

        md = RtReprojectMotionDesc()
        if spheres is not None:
            md.n_spheres, md.spheres, md.keep_spheres, md.prev_spheres, md.keep_prev_spheres = table_pair(
                "spheres", spheres, prev_spheres, SPHERE_DTYPE, "SPHERE_DTYPE")
        if media is not None:
            md.n_media, md.media, md.keep_media = bufs.table(media, "media", MEDIUM_DTYPE, "MEDIUM_DTYPE")
        if md.n_spheres >= 1 << 28 or md.n_media >= 1 << 28:
            raise ValueError("spheres / media: 2^28 records or more")
        md.time = float(np.float32(0.5 * (cur.time0 + cur.time1))) if time is None else float(np.float32(time))
        md.prev_time = float(np.float32(0.5 * (prev.time0 + prev.time1))) if prev_time is None else float(np.float32(prev_time))
        if not np.isfinite(md.time) or not np.isfinite(md.prev_time):
            raise ValueError("time and prev_time must be finite")
        if instances is not None:
            if prev_instances is None:
                raise ValueError("instances needs prev_instances")
            if inst is None:
                raise ValueError("instances: inst is required, it says which instance a pixel shows")
            if (prev_inst is None) != (history is None):
                raise ValueError("instances: prev_inst is required exactly when history is given")
            imd = RtReprojectInstanceDesc()
            imd.n_instances, imd.instances, imd.keep_instances, imd.prev_instances, imd.keep_prev_instances = table_pair(
                "instances", instances, prev_instances, INSTANCE_DTYPE, "INSTANCE_DTYPE")
            if imd.n_instances >= 1 << 28:
                raise ValueError("instances: 2^28 records or more")
        if quads is not None:
            if prev_quads is None:
                raise ValueError("quads needs prev_quads")
            if inst is None:
                raise ValueError("quads: inst is required, it says in whose object space a quad's record lives")
            if (prev_inst is None) != (history is None):
                raise ValueError("quads: prev_inst is required exactly when history is given")
            if imd is None:
                imd = RtReprojectInstanceDesc()
            qmd = RtReprojectQuadDesc()
            qmd.n_quads, qmd.quads, qmd.keep_quads, qmd.prev_quads, qmd.keep_prev_quads = table_pair(
                "quads", quads, prev_quads, QUAD_DTYPE, "QUAD_DTYPE")
            if qmd.n_quads >= 1 << 28:
                raise ValueError("quads: 2^28 records or more")

    d = RtReprojectDesc()
    d.nx, d.ny, d.cur, d.prev = nx, ny, cur, prev
    rgb, one = (ny, nx, 3), (ny, nx)
    adr, f32, i32 = bufs.address, ("float32",), ("int32",)
    d.color, d.depth, d.alpha = adr(color, "color", f32, rgb), adr(depth, "depth", f32, one), adr(alpha, "alpha", f32, one)
    d.normal, d.prim = adr(normal, "normal", f32, rgb), adr(prim, "prim", i32, one)
    d.history, d.history_len = adr(history, "history", f32, rgb), adr(history_len, "history_len", f32, one)
    d.prev_depth, d.prev_alpha = adr(prev_depth, "prev_depth", f32, one), adr(prev_alpha, "prev_alpha", f32, one)
    d.prev_normal, d.prev_prim = adr(prev_normal, "prev_normal", f32, rgb), adr(prev_prim, "prev_prim", i32, one)
    if out is None:
        out = bufs.empty(rgb)
    if out_len is None:
        out_len = bufs.empty(one)
    motion = bufs.empty((ny, nx, 2)) if motion is True else None if motion is False else motion
    d.out, d.out_len, d.motion = adr(out, "out", f32, rgb), adr(out_len, "out_len", f32, one), adr(motion, "motion", f32, (ny, nx, 2))
    d.alpha_min, d.depth_tol, d.normal_min, d.max_history = alpha_min, depth_tol, normal_min, max_history
    if imd is not None:
        imd.inst, imd.prev_inst = adr(inst, "inst", i32, one), adr(prev_inst, "prev_inst", i32, one)
    L, args = rt_lib(), (0 if bufs.on_host else 1, _stream_arg(stream), 1 if blocking else 0)
    if md is None:
        _status(L.rt_reproject(C.byref(d), *args), "rt_reproject")
    elif imd is None:
        _status(L.rt_reproject_moving(C.byref(d), C.byref(md), *args), "rt_reproject_moving")
    elif qmd is None:
        _status(L.rt_reproject_instances(C.byref(d), C.byref(md), C.byref(imd), *args), "rt_reproject_instances")
    else:
        _status(L.rt_reproject_quads(C.byref(d), C.byref(md), C.byref(imd), C.byref(qmd), *args), "rt_reproject_quads")
    return ReprojectResult(out, out_len, motion)


def _chain_args(max_bounces, fuzz_limit):
    """(max_bounces, fuzz_limit) of render_aov_through as rt_aov_through_desc takes them, or ValueError."""
    if isinstance(max_bounces, bool) or not isinstance(max_bounces, (int, np.integer)) or not 0 <= int(max_bounces) <= 16:
        raise ValueError("max_bounces must be an integer in 0..16")
    fuzz_limit = float(fuzz_limit)
    if not (np.isfinite(fuzz_limit) and 0 <= fuzz_limit <= float(np.finfo(np.float32).max)):
        raise ValueError("fuzz_limit must be finite and >= 0")
    return int(max_bounces), fuzz_limit


# the three kinds of record update: the argument's name, its dtype and its structure (whose record pointer carries the name)
_SPHERES = ("spheres", "sphere", SPHERE_DTYPE, "SPHERE_DTYPE", RtSphereUpdate)
_INSTANCES = ("instances", "instance", INSTANCE_DTYPE, "INSTANCE_DTYPE", RtInstanceUpdate)
_QUADS = ("quads", "quad", QUAD_DTYPE, "QUAD_DTYPE", RtQuadUpdate)


def _record_update(kind, records, indices, first, device=None):
    """An RtSphereUpdate / RtInstanceUpdate / RtQuadUpdate over `records` -- host records, or with a `device` a tensor on it as
    well -- and whether they are on the device.  The structure keeps its arrays alive.  ValueError for malformed arguments."""
    name, one, dtype, dtype_name, struct = kind
    bufs = _Buffers(device is None or isinstance(records, np.ndarray), name, device)
    u = struct()
    u.count, address, u.keep_records = bufs.table(records, name, dtype, dtype_name)
    u.first = int(first)
    setattr(u, name, address)
    if indices is not None:
        idx = np.asarray(indices)
        if idx.ndim != 1 or len(idx) != u.count or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f"indices: {u.count} integers are expected, one per record")
        if len(idx) and (idx.min() < -2 ** 31 or idx.max() >= 2 ** 31):
            raise ValueError(f"indices: {one} index out of range")
        u.keep_indices = np.ascontiguousarray(idx, np.int32)
        u.indices = u.keep_indices.ctypes.data
    return u, not bufs.on_host


def _refit(kind, entry, desc, records, indices, first):
    """rt_refit_nodes / rt_refit_instances / rt_refit_quads: (nodes, records) of the description the update is equivalent to."""
    u, _ = _record_update(kind, records, indices, first)
    nodes, out = np.zeros(desc.n_nodes, NODE_DTYPE), np.zeros(getattr(desc, "n_" + kind[0]), kind[2])
    _status(getattr(rt_lib(), entry)(C.byref(desc), C.byref(u), nodes.ctypes.data, out.ctypes.data), entry)
    return nodes, out


def refit_nodes(desc: RtSceneDesc, spheres, indices=None, first: int = 0):
    """rt_refit_nodes, host only: the description that DeviceScene.update_spheres(spheres, indices, first) is equivalent to.
    Returns (nodes, spheres) of it as NODE_DTYPE / SPHERE_DTYPE arrays.  ValueError when the update is refused."""
    return _refit(_SPHERES, "rt_refit_nodes", desc, spheres, indices, first)


def refit_instances(desc: RtSceneDesc, instances, indices=None, first: int = 0):
    """rt_refit_instances, host only: the description that DeviceScene.update_instances(instances, indices, first) is equivalent
    to.  Returns (nodes, instances) of it as NODE_DTYPE / INSTANCE_DTYPE arrays.  ValueError when the update is refused."""
    return _refit(_INSTANCES, "rt_refit_instances", desc, instances, indices, first)


def refit_quads(desc: RtSceneDesc, quads, indices=None, first: int = 0):
    """rt_refit_quads, host only: the description that DeviceScene.update_quads(quads, indices, first) is equivalent to.
    Returns (nodes, quads) of it as NODE_DTYPE / QUAD_DTYPE arrays.  ValueError when the update is refused."""
    return _refit(_QUADS, "rt_refit_quads", desc, quads, indices, first)


def _float3(x, name):
    a = np.asarray(x, np.float32)
    if a.shape != (3,):
        raise ValueError(f"{name}: three numbers are expected")
    return (C.c_float * 3)(*[float(c) for c in a])


def quad_record(Q, u, v, mat: int) -> np.ndarray:
    """One QUAD_DTYPE record (shape (1,)) of quad(Q, u, v) with material index `mat`: D, w and the unit normal come from the
    host library's own quad constructor (the reference's float arithmetic), so the record is what a flattened scene with that
    quad holds.  What DeviceScene.update_quads takes for a quad that moves or changes shape."""
    rec = np.zeros(1, QUAD_DTYPE)
    if host_lib().rtw_quad_record(_float3(Q, "Q"), _float3(u, "u"), _float3(v, "v"), int(mat), rec.ctypes.data) != 0:
        raise RtError("rtw_quad_record failed")
    return rec


def box_records(a, b, mat: int) -> np.ndarray:
    """The six QUAD_DTYPE records, in face order, of make_box(a, b) with material index `mat`, through the host library's own
    make_box: what replaces quads first_quad .. first_quad + 5 of a box that changes size (DeviceScene.update_quads)."""
    rec = np.zeros(6, QUAD_DTYPE)
    if host_lib().rtw_box_records(_float3(a, "a"), _float3(b, "b"), int(mat), rec.ctypes.data) != 0:
        raise RtError("rtw_box_records failed")
    return rec


def instance_record(child: int, angle_degrees=None, offset=None) -> np.ndarray:
    """One INSTANCE_DTYPE record (shape (1,)) of translate(rotate_y(child, angle_degrees), offset), either half left out when
    its argument is None -- at least one must be given.  sin_t and cos_t come from the reference's own float arithmetic
    (rad = angle * 0.017453292519943295769f, then libm's sinf / cosf, through the host library): what a flattened scene with
    that rotation holds.  child: the prim ref the scene holds for the instance (DeviceScene.instances()[i]["child"])."""
    if angle_degrees is None and offset is None:
        raise ValueError("instance_record: an angle, an offset or both are expected")
    rec = np.zeros(1, INSTANCE_DTYPE)
    rec["cos_t"], rec["child"] = 1.0, child
    if angle_degrees is not None:
        s, c = C.c_float(), C.c_float()
        if host_lib().rtw_rotation(float(angle_degrees), C.byref(s), C.byref(c)) != 0:
            raise RtError("rtw_rotation failed")
        rec["sin_t"], rec["cos_t"] = s.value, c.value
        rec["flags"] |= RT_INST_ROTATE_Y
    if offset is not None:
        rec["offset"] = np.asarray(offset, np.float32).reshape(3)
        rec["flags"] |= RT_INST_TRANSLATE
    return rec


class DeviceScene:
    """rt_scene*: the flattened scene resident in HBM."""

    def __init__(self, host_scene: HostScene):
        if _initialised_device is None:
            init(0)
        self.host = host_scene
        self.device = _initialised_device
        self._p = C.c_void_p()
        _check(rt_lib().rt_scene_create(C.byref(host_scene.desc), C.byref(self._p)), "rt_scene_create")

    def set_camera(self, camera: RtCamera, recalibrate: bool = False) -> None:
        """Another view of the scene as it stands on the device (rt_scene_set_camera): every later frame entry writes what it
        would write on a scene created with this camera.  recalibrate=True also renders the small calibration frame again
        for the cost prior of ranked frames; without it the old prior stays, which costs time and never a pixel.  A
        non-finite field or time1 < time0 is ValueError."""
        _status(rt_lib().rt_scene_set_camera(self._p, C.byref(camera), 1 if recalibrate else 0), "rt_scene_set_camera")

    def camera(self) -> RtCamera:
        """The camera the next frame uses (rt_scene_get_camera): the description's, or the last one set."""
        c = RtCamera()
        _check(rt_lib().rt_scene_get_camera(self._p, C.byref(c)), "rt_scene_get_camera")
        return c

    def update_spheres(self, spheres, indices=None, first: int = 0, recalibrate: bool = False, stream=None) -> None:
        """New records for spheres of the scene as it stands on the device (rt_scene_update_spheres): record k replaces sphere
        indices[k], or sphere first + k without indices; the boxes that depend on them are refit on the device and every
        later frame and query is what a scene created from the changed description gives.  recalibrate=True also renders
        the small calibration frame again for the cost prior; without it the prior stays, which costs time and never a pixel.

        spheres: a numpy array of SPHERE_DTYPE -- copied to the device -- or a contiguous torch tensor of shape (count, 8)
        with a 4-byte dtype on the scene's device, read in place: the eight words of rt_sphere per row (view the tensor as
        int32 to set `mat`).  With a tensor the work is enqueued on `stream` (a torch.cuda.Stream; default: the current
        stream); a `stream` other than the current one first waits for the current stream's work.  Either way the call returns
        when the update is complete.  indices: integers, host memory always.  Malformed arguments, an index out of range or
        given twice, a non-finite record, a material out of range and a sphere under an instance raise ValueError before
        anything is launched; a bad record in a device tensor raises it after the others were applied."""
        self._update_records(_SPHERES, "rt_scene_update_spheres", spheres, indices, first, recalibrate, stream)

    def update_instances(self, instances, indices=None, first: int = 0, recalibrate: bool = False, stream=None) -> None:
        """New records for instances of the scene as it stands on the device (rt_scene_update_instances): record k replaces
        instance indices[k], or instance first + k without indices; sin_t, cos_t, offset and flags (1, 2 or 3) may change, child
        must be the scene's own (see instance_record).  The boxes that depend on them are refit on the device and every later
        frame and query is what a scene created from the changed description gives.  recalibrate: as update_spheres.

        instances: a numpy array of INSTANCE_DTYPE -- copied to the device -- or a contiguous torch tensor of shape (count, 8),
        float32 or int32, on the scene's device, read in place: the eight words of rt_instance per row.  stream, indices and the
        argument errors are update_spheres'.  An index out of range or given twice, a non-finite record, bad flags and another
        child raise ValueError before anything is launched; a bad record in a device tensor raises it after the others were
        applied."""
        self._update_records(_INSTANCES, "rt_scene_update_instances", instances, indices, first, recalibrate, stream)

    def update_quads(self, quads, indices=None, first: int = 0, recalibrate: bool = False, stream=None) -> None:
        """New records for quads of the scene as it stands on the device (rt_scene_update_quads): record k replaces quad
        indices[k], or quad first + k without indices -- free quads and the faces of boxes (quads first_quad .. first_quad + 5),
        under an instance or not.  Q, D, u, v, w, n and mat may change; D, w and n are the caller's, as in a description (see
        quad_record and box_records).  The boxes that depend on the quads are refit on the device, the axis-aligned marks the
        scene keeps follow, and every later frame and query is what a scene created from the changed description gives.
        recalibrate: as update_spheres.

        quads: a numpy array of QUAD_DTYPE -- copied to the device -- or a contiguous torch tensor of shape (count, 20) with a
        4-byte dtype on the scene's device, read in place: the twenty words of rt_quad per row.  stream, indices and the argument
        errors are update_spheres'.  An index out of range or given twice, a non-finite record and a material out of range raise
        ValueError before anything is launched; a bad record in a device tensor raises it after the others were applied."""
        self._update_records(_QUADS, "rt_scene_update_quads", quads, indices, first, recalibrate, stream)

    def _update_records(self, kind, entry, records, indices, first, recalibrate, stream):
        if isinstance(records, np.ndarray) and stream is not None:
            raise ValueError("stream: only a device tensor is enqueued on a torch stream")
        u, on_device = _record_update(kind, records, indices, first, self.device)
        stream_p = None
        if on_device:
            if u.count == 0:
                return
            stream_p = C.c_void_p(_enqueue_on(records.device, stream, [records]).cuda_stream)
        _status(getattr(rt_lib(), entry)(self._p, C.byref(u), 1 if on_device else 0, 1 if recalibrate else 0, stream_p), entry)

    def spheres(self) -> np.ndarray:
        """The sphere records the next frame uses (rt_scene_get_spheres): the description's, with every update applied."""
        out = np.zeros(self.host.desc.n_spheres, SPHERE_DTYPE)
        _check(rt_lib().rt_scene_get_spheres(self._p, out.ctypes.data, len(out)), "rt_scene_get_spheres")
        return out

    def instances(self) -> np.ndarray:
        """The instance records the next frame uses (rt_scene_get_instances): the description's, with every update applied."""
        out = np.zeros(self.host.desc.n_instances, INSTANCE_DTYPE)
        _check(rt_lib().rt_scene_get_instances(self._p, out.ctypes.data, len(out)), "rt_scene_get_instances")
        return out

    def quads(self) -> np.ndarray:
        """The quad records the next frame uses (rt_scene_get_quads): the description's, with every update applied; pad0 is 0."""
        out = np.zeros(self.host.desc.n_quads, QUAD_DTYPE)
        _check(rt_lib().rt_scene_get_quads(self._p, out.ctypes.data, len(out)), "rt_scene_get_quads")
        return out

    def debug_quads(self):
        """rt_debug_scene_quads (tests): the device's quad records and box words raw -- pad0 holds the axis code as integer bits,
        bit 30 of a box word the canonical mark.  Returns (QUAD_DTYPE array, int32 array)."""
        quads, boxes = np.zeros(self.host.desc.n_quads, QUAD_DTYPE), np.zeros(self.host.desc.n_boxes, np.int32)
        _check(rt_lib().rt_debug_scene_quads(self._p, quads.ctypes.data if len(quads) else None, len(quads),
                                             boxes.ctypes.data if len(boxes) else None, len(boxes)), "rt_debug_scene_quads")
        return quads, boxes

    COST_MAP_STATES = ("none", "exact", "stale")

    def cost_map(self):
        """The scene's cost map (rt_debug_cost_map): (state, map, parts) -- state "none", "exact" or "stale" for the scene and the
        options as they are now, map the rays per local pixel of the last ranked frame as a (local_rows, nx) uint32 array (None
        with "none"), parts the number of parts the last ranked frame ran as.  Closes a pending frame."""
        L = rt_lib()
        info = (C.c_int32 * 4)()
        _check(L.rt_debug_cost_map(self._p, None, 0, info), "rt_debug_cost_map")
        if info[0] == 0:
            return "none", None, int(info[3])
        out = np.zeros((int(info[2]), int(info[1])), np.uint32)
        _check(L.rt_debug_cost_map(self._p, out.ctypes.data, out.size, info), "rt_debug_cost_map")
        return self.COST_MAP_STATES[info[0]], out, int(info[3])

    def handoff_queue(self):
        """The tail hand-off queue of the last frame's last part in push order (rt_debug_handoff_queue): (entries, costs, served, info) --
        uint64 (next sample << 32 | pixel); entry for entry the pixel's parked cost; the queue as the tail launch was given it; and
        dict(ordered: the ordering kernels ran, min, max: the entry counts between which they order and outside which they copy)."""
        L = rt_lib()
        L.rt_debug_handoff_queue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        info = (C.c_int64 * 4)()
        _check(L.rt_debug_handoff_queue(self._p, None, None, None, 0, info), "rt_debug_handoff_queue")
        n = int(info[0])
        entries, costs, served = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        if n:
            _check(L.rt_debug_handoff_queue(self._p, entries.ctypes.data, costs.ctypes.data, served.ctypes.data, n, info), "rt_debug_handoff_queue")
        return entries, costs, served, dict(ordered=bool(info[1]), min=int(info[2]), max=int(info[3]))

    def set_cost_map(self, costs) -> None:
        """Install `costs` (one uint32 per local pixel of the last ranked frame) as that frame geometry's exact cost map
        (rt_debug_set_cost_map).  Any map schedules the next frame; none changes a pixel."""
        a = np.ascontiguousarray(costs, np.uint32)
        _check(rt_lib().rt_debug_set_cost_map(self._p, a.ctypes.data, a.size), "rt_debug_set_cost_map")

    def render(self, frame: RtFrameDesc, out=None, stream: int = 0, blocking: bool = True):
        """Render into `out`: a float32 numpy array (host) or an integer device pointer.  Returns (array|None, stats)."""
        L = rt_lib()
        rows = L.rt_frame_local_rows(C.byref(frame))
        if rows < 0:
            raise RtError("bad row partition")
        stats = RtStats()
        if out is None:
            out = np.empty((rows, frame.nx, 3), np.float32)
        if isinstance(out, np.ndarray):
            assert out.dtype == np.float32 and out.size == rows * frame.nx * 3 and out.flags["C_CONTIGUOUS"]
            _check(L.rt_render(self._p, C.byref(frame), out.ctypes.data, 0, stream, 1, C.byref(stats)), "rt_render")
            return out, stats
        _check(L.rt_render(self._p, C.byref(frame), C.c_void_p(int(out)), 1, stream, 1 if blocking else 0, C.byref(stats)), "rt_render")
        return None, stats

    def _ray_buffers(self, origins, directions):
        """The buffer rule of trace() and radiance(), whose anchor is `origins` (N, 3) on this scene's device, and N."""
        bufs = _Buffers(isinstance(origins, np.ndarray), "origins", self.device)
        if not (bufs.on_host or hasattr(origins, "data_ptr")):
            raise bufs.wrong_kind("origins", "a numpy array")
        if origins.ndim != 2 or origins.shape[1] != 3:
            raise ValueError(f"origins: shape {tuple(origins.shape)}, expected (N, 3)")
        if directions is None:
            raise ValueError("directions are required")
        return bufs, int(origins.shape[0])

    def trace(self, origins, directions, times=None, tmin: float = 0.001, tmax=None, any_hit: bool = False, record: bool = False,
              stream=None):
        """Batched ray queries (rt_trace_rays): the closest hit -- or, with any_hit, whether anything is hit -- of every ray
        in its window (tmin, tmax), applied by each object as the reference's hit function applies it (include/rt_abi.h).

        origins, directions: (N, 3) float32; times, tmax: (N,) float32 or None (0 / FLT_MAX for every ray).  Either all
        torch tensors on this scene's device -- used in place (made contiguous if they are not), outputs are tensors on the
        device, the work is enqueued on `stream` (a torch.cuda.Stream; default: the current stream) and the call does not
        wait; a `stream` other than the current one first waits for the current stream's work, and the caller orders any
        later use of the outputs after `stream` -- or all numpy arrays -- copied to the device through torch, outputs are numpy arrays and the call waits.
        Returns a TraceResult (t: FLT_MAX on a miss, prim: RT_PRIM_REF or -1, inst: instance index or -1; point, normal,
        uv, mat only with record=True, zeros and mat = -1 on a miss), or with any_hit a bool array (record must then be False).  Malformed input raises
        ValueError before anything is launched.  A ray whose tmax is NaN, or with a NaN or infinite component in its origin,
        direction or time, is a miss."""
        import torch
        if any_hit and record:
            raise ValueError("any_hit returns hit flags only: record=True needs a closest-hit query")
        bufs, n = self._ray_buffers(origins, directions)
        on_host, dev = bufs.on_host, bufs.torch_device()
        if not np.isfinite(tmin):
            raise ValueError("tmin must be finite")
        ins = [origins, directions, times, tmax]
        for k, x in zip(("origins", "directions", "times", "tmax"), ins):
            bufs.address(x, k, shape=(n, 3) if k in ("origins", "directions") else (n,), strided=True)
        ins = [None if x is None else (torch.from_numpy(np.ascontiguousarray(x)).to(dev) if on_host else x.contiguous()) for x in ins]

        def empty(shape, dtype):
            return torch.empty(shape, dtype=dtype, device=dev)
        if any_hit:
            outs = {"hit_out": empty((n,), torch.uint8)}
        else:
            outs = {"t_out": empty((n,), torch.float32), "prim_out": empty((n,), torch.int32), "inst_out": empty((n,), torch.int32)}
            if record:
                outs.update(point_out=empty((n, 3), torch.float32), normal_out=empty((n, 3), torch.float32),
                            uv_out=empty((n, 2), torch.float32), mat_out=empty((n,), torch.int32))
        stream = _enqueue_on(dev, stream, ins + list(outs.values()) if n > 0 else ())
        if n > 0:
            b = RtRayBatch()
            b.n = n
            b.origins, b.directions, b.times, b.tmax = (None if x is None else x.data_ptr() for x in ins)
            b.tmin = float(tmin)
            b.mode = RT_TRACE_ANY if any_hit else RT_TRACE_CLOSEST
            for k, v in outs.items():
                setattr(b, k, v.data_ptr())
            _check(rt_lib().rt_trace_rays(self._p, C.byref(b), C.c_void_p(stream.cuda_stream), 0), "rt_trace_rays")
        if on_host:
            stream.synchronize()
            outs = {k: v.cpu().numpy() for k, v in outs.items()}
        if any_hit:
            h = outs["hit_out"]
            return h.view(np.bool_) if on_host else h.view(torch.bool)
        return TraceResult(outs["t_out"], outs["prim_out"], outs["inst_out"], outs.get("point_out"), outs.get("normal_out"),
                           outs.get("uv_out"), outs.get("mat_out"))

    def radiance(self, origins, directions, times=None, ns: int = 1, seeds=None, seed_base: int = 1984, background=None, gradient=None,
                 count_rays: bool = False, stream=None):
        """Radiance queries (rt_radiance_rays): the path-traced colour along every ray, `ns` samples each -- per ray what
        rt_render writes, at gamma 1, for the one pixel of a camera that sends every sample along that ray (include/rt_abi.h).

        origins, directions: (N, 3) float32; times: (N,) float32 or None (0 for every ray); seeds: (N,) int64 or uint64 (the
        bits are the seed) or None (seed_base + i).  background: three floats, gradient: bool; None = the host scene's.
        Tensors or numpy arrays, streams and waiting as in trace().  Returns a RadianceResult (rgb: (N, 3) float32; rays: (N,)
        int32 holding each query's ray count, only with count_rays=True).  Malformed input raises ValueError before anything
        is launched.  A ray with a NaN or infinite component in its origin, direction or time, or with a zero direction,
        gets zeros and 0 rays."""
        import torch
        bufs, n = self._ray_buffers(origins, directions)
        on_host, dev = bufs.on_host, bufs.torch_device()
        if isinstance(ns, bool) or not isinstance(ns, (int, np.integer)) or not 1 <= int(ns) <= 1 << 20:
            raise ValueError("ns must be an integer in 1 .. 1 << 20")
        if isinstance(seed_base, bool) or not isinstance(seed_base, (int, np.integer)) or not 0 <= int(seed_base) < 1 << 64:
            raise ValueError("seed_base must be an integer in 0 .. 2**64 - 1")
        bg = self.host.background if background is None else [float(x) for x in np.asarray(background, np.float64).reshape(-1)]
        if len(bg) != 3:
            raise ValueError("background: three floats are expected")
        gradient = self.host.use_gradient_bg if gradient is None else gradient
        ins = [origins, directions, times, seeds]
        for k, x in zip(("origins", "directions", "times", "seeds"), ins):
            bufs.address(x, k, ("int64", "uint64") if k == "seeds" else ("float32",), (n, 3) if k in ("origins", "directions") else (n,), strided=True)
        if on_host:   # (torch has no uint64 arithmetic to speak of: the seeds travel as their int64 bits)
            ins = [None if x is None else torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else np.ascontiguousarray(x)).to(dev)
                   for x in ins]
        else:
            ins = [None if x is None else x.contiguous() for x in ins]
        outs = {"rgb_out": torch.empty((n, 3), dtype=torch.float32, device=dev)}
        if count_rays:
            outs["rays_out"] = torch.empty((n,), dtype=torch.int32, device=dev)
        stream = _enqueue_on(dev, stream, ins + list(outs.values()) if n > 0 else ())
        if n > 0:
            b = RtRadianceBatch()
            b.n = n
            b.origins, b.directions, b.times, b.seeds = (None if x is None else x.data_ptr() for x in ins)
            b.seed_base, b.ns = int(seed_base), int(ns)
            b.background[:] = bg
            b.use_gradient_bg = 1 if gradient else 0
            for k, v in outs.items():
                setattr(b, k, v.data_ptr())
            _status(rt_lib().rt_radiance_rays(self._p, C.byref(b), C.c_void_p(stream.cuda_stream), 0), "rt_radiance_rays")
        if on_host:
            stream.synchronize()
            outs = {k: v.cpu().numpy() for k, v in outs.items()}
        return RadianceResult(outs["rgb_out"], outs.get("rays_out"))

    def render_aov(self, frame: RtFrameDesc, albedo: bool = True, normal: bool = True, depth: bool = True, alpha: bool = True,
                   ids: bool = False, out=None, stream=0, blocking: bool = True) -> dict:
        """Feature buffers of `frame` (rt_render_aov): per pixel the albedo, normal, depth (the ray parameter t) and coverage
        of the primary rays' first hits, averaged over the frame's ns samples, and with ids=True the first sample's prim,
        inst and mat (-1 on a miss) -- what a denoiser or a compositor wants beside a noisy frame (include/rt_abi.h).

        out=None: a dict of numpy arrays for the selected outputs, rows x nx (x 3), float32 (ids: int32); the call waits.
        out = a dict whose keys are output names (AOV_OUTPUTS): those outputs are written in place and the flags are not
        looked at -- all numpy arrays (the call waits), or all contiguous torch tensors on this scene's device, zero-copy,
        enqueued on `stream` (a hipStream_t as an integer or a torch.cuda.Stream) and waited for only with blocking=True.
        Returns the dict.  Malformed arguments raise ValueError before anything is launched."""
        names = [k for k, on in (("albedo", albedo), ("normal", normal), ("depth", depth), ("alpha", alpha)) if on]
        names += ["prim", "inst", "mat"] if ids else []
        return self._aov_call(frame, names, out, None, stream, blocking)

    def _aov_call(self, frame, names, out, chain, stream, blocking) -> dict:
        """render_aov (chain None) and render_aov_through (chain = (max_bounces, fuzz_limit)): the outputs `names`, or `out`."""
        L = rt_lib()
        table = AOV_OUTPUTS if chain is None else AOV_THROUGH_OUTPUTS
        rows = L.rt_frame_local_rows(C.byref(frame))
        if frame.nx <= 0 or frame.ny <= 0 or frame.ns <= 0 or rows < 0:
            raise ValueError("bad frame size, sample count or row partition")
        if out is None:
            out = {k: np.empty((rows, frame.nx, 3) if table[k][0] == 3 else (rows, frame.nx), table[k][1]) for k in names}
        if not isinstance(out, dict) or not out:
            raise ValueError("no output is requested")
        bufs = _Buffers(all(isinstance(v, np.ndarray) for v in out.values()), "out", self.device)
        a, t = RtAovDesc(), RtAovThroughDesc()
        for k, v in out.items():
            if k not in table:
                raise ValueError(f"unknown output '{k}': one of {', '.join(table)} is expected")
            if not bufs.on_host and not hasattr(v, "data_ptr"):
                raise ValueError("out: all numpy arrays or all torch tensors are expected")
            ch, dtype = table[k]
            setattr(a if k in AOV_OUTPUTS else t, k, bufs.address(v, k, (np.dtype(dtype).name,), count=rows * frame.nx * ch))
        args = (0 if bufs.on_host else 1, _stream_arg(stream), 1 if blocking else 0)
        if chain is None:
            st = L.rt_render_aov(self._p, C.byref(frame), C.byref(a), *args)
        else:
            t.max_bounces, t.fuzz_limit = chain
            st = L.rt_render_aov_through(self._p, C.byref(frame), C.byref(a), C.byref(t), *args)
        _status(st, "rt_render_aov" if chain is None else "rt_render_aov_through")
        return out

    def render_aov_through(self, frame: RtFrameDesc, max_bounces: int = AOV_THROUGH_DEFAULTS["max_bounces"],
                           fuzz_limit: float = AOV_THROUGH_DEFAULTS["fuzz_limit"], albedo: bool = True, normal: bool = True,
                           depth: bool = True, alpha: bool = True, ids: bool = False, through: bool = False, bounces: bool = False,
                           out=None, stream=0, blocking: bool = True) -> dict:
        """Feature buffers of `frame` at the first non-specular surface (rt_render_aov_through): every sample of render_aov is
        followed through glass (refracted, or mirrored under total internal reflection) and off metals whose fuzz is at most
        fuzz_limit, for at most max_bounces (0..16) bounces; albedo is the surface's where the chain ends times the tint of the
        mirrors on the way, normal is that surface's, depth the whole way in the primary ray's parameter (include/rt_abi.h).
        through=True adds the share of the pixel's samples that followed at least one bounce, bounces=True the first
        sample's bounce count (int32).  max_bounces=0 is render_aov.

        out, stream, blocking and the returned dict: as render_aov, with the keys of AOV_THROUGH_OUTPUTS.  Malformed arguments
        raise ValueError before anything is launched."""
        chain = _chain_args(max_bounces, fuzz_limit)
        names = [k for k, on in (("albedo", albedo), ("normal", normal), ("depth", depth), ("alpha", alpha)) if on]
        names += ["prim", "inst", "mat"] if ids else []
        names += [k for k, on in (("through", through), ("bounces", bounces)) if on]
        return self._aov_call(frame, names, out, chain, stream, blocking)

    def render_denoised(self, frame: RtFrameDesc, variance: bool = False, batches=None, through: bool = False,
                        max_bounces: int = AOV_THROUGH_DEFAULTS["max_bounces"], fuzz_limit: float = AOV_THROUGH_DEFAULTS["fuzz_limit"],
                        **denoise_args) -> dict:
        """A denoised frame: render() of `frame` at gamma 1, render_aov() of it (albedo, normal, depth at min(frame.ns, 16)
        samples) and denoise() of the two (its keyword arguments pass through).  Returns {"color": the denoised linear
        frame, "noisy": the render, "albedo", "normal", "depth"} as numpy arrays.  The frame must be the whole image: a
        partitioned one is ValueError.

        variance=True: the frame comes from render_variance() -- `batches` batches, by default the largest divisor of
        frame.ns in 2..16 (a frame.ns without one, such as 1 or 17, is ValueError: pass batches) -- and the filter runs variance-guided
        (denoise(variance=...)); the result also holds "variance", the render's per-pixel variance.

        through=True: the guides come from render_aov_through(max_bounces, fuzz_limit) -- the surfaces seen through glass and
        in mirrors -- instead of render_aov."""
        if frame.nx <= 0 or frame.ny <= 0 or frame.ns <= 0:
            raise ValueError("bad frame size or sample count")
        if frame.tile_first != 0 or frame.tile_stride != 1 or frame.tile_rows < frame.ny:
            raise ValueError("render_denoised needs the whole frame (tile_rows >= ny, tile_first = 0, tile_stride = 1)")
        if not variance and batches is not None:
            raise ValueError("batches needs variance=True")
        if through:
            max_bounces, fuzz_limit = _chain_args(max_bounces, fuzz_limit)
        f = RtFrameDesc.from_buffer_copy(frame)
        f.gamma = 1.0
        var = None
        if variance:
            if batches is None:
                batches = min(frame.ns, 16)
                while frame.ns % batches:
                    batches -= 1
                if batches < 2:
                    raise ValueError(f"frame.ns = {frame.ns} has no divisor in 2..16: pass batches (2..64, a divisor of frame.ns)")
            noisy, var, _ = self.render_variance(f, batches)
        else:
            noisy, _ = self.render(f)
        f.ns = min(frame.ns, 16)
        aov = self.render_aov_through(f, max_bounces, fuzz_limit, alpha=False) if through else self.render_aov(f, alpha=False)
        if variance:
            denoise_args = dict(denoise_args, variance=var)
        color = denoise(noisy, aov["albedo"], aov["normal"], aov["depth"], **denoise_args)
        r = {"color": color, "noisy": noisy, "albedo": aov["albedo"], "normal": aov["normal"], "depth": aov["depth"]}
        if variance:
            r["variance"] = var
        return r

    def render_upscaled(self, frame: RtFrameDesc, factor: int = 2, denoise: bool = True, **args) -> dict:
        """The nx x ny frame of `frame` from paths traced at nx/factor x ny/factor: render() of the coarse frame at gamma 1,
        render_aov() of it (albedo, normal, depth at min(frame.ns, 16) samples), with denoise=True denoise() of the coarse
        frame with its own guides, render_aov() of the full frame at min(frame.ns, 16) samples, and upscale() of the lot.
        Keyword arguments named denoise_* go to denoise() with the prefix stripped, the others to upscale().

        frame.ns is the COARSE frame's sample count: a coarse frame has 1 / factor^2 of the pixels, so equal path cost with a
        full-resolution render at n samples is ns = n * factor^2.  The frame must be the whole nx x ny image with nx and ny
        multiples of factor, otherwise ValueError.

        Returns {"color": the upscaled linear frame (ny, nx, 3), "low": the coarse frame that was upscaled (denoised when
        denoise), "albedo", "normal", "depth": the full-resolution guides, "weight": upscale()'s weight_out} as numpy
        arrays, and with denoise=True "noisy_low", the coarse render before the filter."""
        if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or not 2 <= int(factor) <= 8:
            raise ValueError("factor must be an integer in 2..8")
        factor = int(factor)
        if frame.nx <= 0 or frame.ny <= 0 or frame.ns <= 0:
            raise ValueError("bad frame size or sample count")
        if frame.tile_first != 0 or frame.tile_stride != 1 or frame.tile_rows < frame.ny:
            raise ValueError("render_upscaled needs the whole frame (tile_rows >= ny, tile_first = 0, tile_stride = 1)")
        if frame.nx % factor or frame.ny % factor:
            raise ValueError(f"render_upscaled needs nx and ny to be multiples of factor = {factor}")
        denoise_args = {k[len("denoise_"):]: v for k, v in args.items() if k.startswith("denoise_")}
        upscale_args = {k: v for k, v in args.items() if not k.startswith("denoise_")}
        lo = RtFrameDesc.from_buffer_copy(frame)
        lo.nx, lo.ny, lo.gamma = frame.nx // factor, frame.ny // factor, 1.0
        lo.tile_rows = lo.ny
        noisy, _ = self.render(lo)
        lo.ns = min(frame.ns, 16)
        g_lo = self.render_aov(lo, alpha=False)
        low = _denoise(noisy, g_lo["albedo"], g_lo["normal"], g_lo["depth"], **denoise_args) if denoise else noisy
        full = RtFrameDesc.from_buffer_copy(frame)
        full.ns, full.gamma = min(frame.ns, 16), 1.0
        g = self.render_aov(full, alpha=False)
        weight = np.empty((frame.ny, frame.nx), np.float32)
        color = upscale(low, factor, g_lo["albedo"], g_lo["normal"], g_lo["depth"], g["albedo"], g["normal"], g["depth"], weight_out=weight,
                        **upscale_args)
        r = {"color": color, "low": low, "albedo": g["albedo"], "normal": g["normal"], "depth": g["depth"], "weight": weight}
        if denoise:
            r["noisy_low"] = noisy
        return r

    def render_variance(self, frame: RtFrameDesc, batches: int, out=None, variance_out=None, stream=0):
        """A frame and the variance of each of its pixels (rt_render_variance): fb is render()'s frame at frame.ns samples, and
        variance (rows x nx) estimates, from the spread of `batches` batch averages, the variance of the pixel's mean of
        r + g + b (include/rt_abi.h).  2 <= batches <= 64 and frame.ns a multiple of it.

        out / variance_out: None (numpy arrays are made), float32 numpy arrays of rows x nx (x 3), or device memory of this
        scene's device -- torch tensors or integer pointers; both host or both device.  stream: a hipStream_t as an integer
        or a torch.cuda.Stream.  The call returns when the frame is complete.  Returns (fb, variance, stats); fb / variance are
        what was passed in (None where an integer pointer was).  Malformed arguments raise ValueError before anything is
        launched."""
        if isinstance(batches, bool) or not isinstance(batches, (int, np.integer)):
            raise ValueError("batches must be an integer")
        batches = int(batches)
        if not 2 <= batches <= 64:
            raise ValueError("batches must be in 2..64")
        if frame.ns <= 0 or frame.ns % batches:
            raise ValueError("frame.ns must be a positive multiple of batches")
        L = rt_lib()
        rows = L.rt_frame_local_rows(C.byref(frame))
        if frame.nx <= 0 or frame.ny <= 0 or rows < 0:
            raise ValueError("bad frame size or row partition")
        if out is None and variance_out is None:
            out = np.empty((rows, frame.nx, 3), np.float32)
            variance_out = np.empty((rows, frame.nx), np.float32)
        if out is None or variance_out is None:
            raise ValueError("out and variance_out go together: pass both or neither")
        bufs = _Buffers(isinstance(out, np.ndarray), "out", self.device)
        if isinstance(variance_out, np.ndarray) != bufs.on_host:
            raise ValueError("out and variance_out must both be host (numpy) or both device memory")
        p_fb = bufs.address(out, "out", count=rows * frame.nx * 3, pointer=True)
        p_var = bufs.address(variance_out, "variance_out", count=rows * frame.nx, pointer=True)
        v = RtVarianceDesc(batches, 0)
        stats = RtStats()
        _status(L.rt_render_variance(self._p, C.byref(frame), C.byref(v), C.c_void_p(p_fb), 0 if bufs.on_host else 1, C.c_void_p(p_var),
                                     _stream_arg(stream), C.byref(stats)), "rt_render_variance")
        ret = lambda x: x if (isinstance(x, np.ndarray) or hasattr(x, "data_ptr")) else None   # noqa: E731
        return ret(out), ret(variance_out), stats

    def render_adaptive(self, frame: RtFrameDesc, min_spp: int, max_spp: int, threshold: float, floor: float = 0.01, out=None,
                        spp_out=None, stream=0):
        """Adaptive sampling (rt_render_adaptive): each pixel stops at the first checkpoint min_spp * 2^k where its average
        moved by at most threshold * (brightness + floor) since the previous checkpoint, else at max_spp (include/rt_abi.h).

        out / spp_out: None (numpy arrays are made), float32 / int32 numpy arrays of rows x nx (x 3), or device memory of
        this scene's device -- torch tensors or integer pointers, both or neither.  stream: a hipStream_t as an integer or a
        torch.cuda.Stream.  The call returns when the frame is complete.  Returns (fb, spp, stats); fb / spp are what was
        passed in (None where an integer pointer was).  Malformed arguments raise ValueError before anything is launched."""
        vals = {"min_spp": min_spp, "max_spp": max_spp}
        for k, v in vals.items():
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{k} must be an integer")
        min_spp, max_spp = int(min_spp), int(max_spp)
        if min_spp < 2 or min_spp % 2:
            raise ValueError("min_spp must be even and >= 2")
        if max_spp < min_spp or max_spp % min_spp or (max_spp // min_spp) & (max_spp // min_spp - 1) or max_spp // min_spp > 1 << 16:
            raise ValueError("max_spp must be min_spp * 2**K with 0 <= K <= 16")
        threshold, floor = float(threshold), float(floor)
        f32_max = float(np.finfo(np.float32).max)   # (the descriptor holds float32: a larger double would become infinite)
        if not np.isfinite(threshold) or abs(threshold) > f32_max:
            raise ValueError("threshold must be finite")
        if not np.isfinite(floor) or floor > f32_max or floor < 0:
            raise ValueError("floor must be finite and >= 0")
        L = rt_lib()
        rows = L.rt_frame_local_rows(C.byref(frame))
        if frame.nx <= 0 or frame.ny <= 0 or rows < 0:
            raise ValueError("bad frame size or row partition")
        if out is None:
            out = np.empty((rows, frame.nx, 3), np.float32)
            if spp_out is None:
                spp_out = np.empty((rows, frame.nx), np.int32)
        bufs = _Buffers(isinstance(out, np.ndarray), "out", self.device)
        if spp_out is not None and isinstance(spp_out, np.ndarray) != bufs.on_host:
            raise ValueError("out and spp_out must both be host (numpy) or both device memory")
        p_fb = bufs.address(out, "out", count=rows * frame.nx * 3, pointer=True)
        p_spp = bufs.address(spp_out, "spp_out", ("int32",), count=rows * frame.nx, pointer=True)
        a = RtAdaptiveDesc(min_spp, max_spp, threshold, floor)
        stats = RtStats()
        _status(L.rt_render_adaptive(self._p, C.byref(frame), C.byref(a), C.c_void_p(p_fb), 0 if bufs.on_host else 1,
                                     C.c_void_p(p_spp) if p_spp else None, _stream_arg(stream), C.byref(stats)), "rt_render_adaptive")
        ret = lambda x: x if (x is None or isinstance(x, np.ndarray) or hasattr(x, "data_ptr")) else None   # noqa: E731
        return ret(out), ret(spp_out), stats

    def adaptive_passes(self) -> list:
        """The passes of the last adaptive frame (diagnostics): dicts of route ("main" / "tier"), active pixels, samples, device ms."""
        buf = np.zeros((32, 5), np.int64)
        n = rt_lib().rt_debug_adaptive_passes(self._p, buf.ctypes.data, 32)
        return [{"route": "tier" if r[0] else "main", "active": int(r[1]), "samples": [int(r[2]), int(r[3])], "ms": r[4] / 1000.0}
                for r in buf[:max(n, 0)]]

    def progressive(self, frame: RtFrameDesc) -> "ProgressiveFrame":
        """Progressive accumulation of `frame` (rt_render_window): windows of samples, a displayable frame after each."""
        return ProgressiveFrame(self, frame)

    def walk_info(self) -> dict:
        """Node counts of the reference tree / the walk array and expected box tests per ray on the calibration frame."""
        a, b, x, y = C.c_int32(0), C.c_int32(0), C.c_double(0), C.c_double(0)
        _check(rt_lib().rt_scene_walk_info(self._p, C.byref(a), C.byref(b), C.byref(x), C.byref(y)), "rt_scene_walk_info")
        return {"nodes_reference": a.value, "nodes_walked": b.value, "tests_before": x.value, "tests_after": y.value}

    def tier_room(self) -> dict:
        """The tier kernel's room as rt_render plans it under the current options (rt_debug_tier_room; nothing is launched)."""
        out = (C.c_int32 * 4)()
        _status(rt_lib().rt_debug_tier_room(self._p, out), "rt_debug_tier_room")
        return {"fits": bool(out[0]), "lds_scene": bool(out[1]), "lds": int(out[2]), "tail_grid": int(out[3])}

    def finish(self) -> RtStats:
        stats = RtStats()
        _check(rt_lib().rt_frame_finish(self._p, C.byref(stats)), "rt_frame_finish")
        return stats

    def close(self):
        if self._p:
            rt_lib().rt_scene_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ProgressiveFrame:
    """rt_progressive_state_* + rt_render_window: the per-pixel XORWOW state and colour sum carried between windows."""

    def __init__(self, scene: DeviceScene, frame: RtFrameDesc):
        self.scene, self.frame = scene, frame
        self._p = C.c_void_p()
        _check(rt_lib().rt_progressive_state_create(scene._p, C.byref(frame), C.byref(self._p)), "rt_progressive_state_create")
        self.rows = rt_lib().rt_frame_local_rows(C.byref(frame))

    def render(self, sample_begin: int, sample_end: int):
        """Samples [sample_begin, sample_end) of every pixel; returns (the frame averaged over sample_end samples, stats)."""
        out = np.empty((self.rows, self.frame.nx, 3), np.float32)
        stats = RtStats()
        _check(rt_lib().rt_render_window(self.scene._p, C.byref(self.frame), out.ctypes.data, 0, self._p, sample_begin, sample_end, None, 1, C.byref(stats)), "rt_render_window")
        return out, stats

    def close(self):
        if self._p:
            rt_lib().rt_progressive_state_destroy(self.scene._p, self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TemporalAccumulator:
    """Frames of a moving camera accumulated over time: push(camera) sets the camera, renders `frame` at gamma 1, takes the
    feature buffers of render_aov (normal, depth, alpha and the ids, at min(frame.ns, 16) samples), reprojects the history
    kept from the last push into the new view (reproject(), normals and ids on) and keeps the result and the buffers for the
    next push.  Returns the accumulated linear frame (ny, nx, 3) as a numpy array -- with denoise=True filtered by denoise()
    with the albedo, normal and depth of the same pass; the history itself stays unfiltered.  **params: thresholds of
    REPROJECT_DEFAULTS.  `frame` must be the whole image.  `length` holds the last push's per-pixel history length.

    follow_spheres=True: the history follows spheres that moved between two pushes (reproject(spheres=...)).  push() then also
    takes an update (spheres, indices, first: DeviceScene.update_spheres' arguments) that it applies first, reads the scene's
    records back (32 bytes per sphere) and reprojects with them, the previous push's records and the scene's media; updates
    the caller made on the scene between two pushes are followed just the same.

    follow_instances=True: likewise for instances (reproject(instances=...)).  push() takes an update (instances,
    instance_indices, instance_first: DeviceScene.update_instances' arguments) that it applies first, reads the scene's instance
    records back, keeps them and render_aov's `inst` with the push, and reprojects with both pushes' records and planes.  The two
    flags combine.

    follow_quads=True: likewise for quads and the faces of boxes (reproject(quads=...)).  push() takes an update (quads,
    quad_indices, quad_first: DeviceScene.update_quads' arguments) that it applies first, reads the scene's quad records back
    and keeps them with the push.  It reads the instance records and `inst` as follow_instances does, whether or not that flag
    is set: a quad under an instance is carried in that instance's object space even when the instance stands still (and an
    instance the caller moved is then followed as well).  The three flags combine."""

    def __init__(self, scene: "DeviceScene", frame: RtFrameDesc, denoise: bool = False, follow_spheres: bool = False,
                 follow_instances: bool = False, follow_quads: bool = False, **params):
        unknown = set(params) - set(REPROJECT_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown parameter(s) {sorted(unknown)}: one of {', '.join(REPROJECT_DEFAULTS)} is expected")
        if frame.nx <= 0 or frame.ny <= 0 or frame.ns <= 0:
            raise ValueError("bad frame size or sample count")
        if frame.tile_first != 0 or frame.tile_stride != 1 or frame.tile_rows < frame.ny:
            raise ValueError("TemporalAccumulator needs the whole frame (tile_rows >= ny, tile_first = 0, tile_stride = 1)")
        self.scene, self.denoise, self.params = scene, bool(denoise), dict(REPROJECT_DEFAULTS, **params)
        self.follow_spheres, self.follow_instances, self.follow_quads = bool(follow_spheres), bool(follow_instances), bool(follow_quads)
        self.frame = RtFrameDesc.from_buffer_copy(frame)
        self.frame.gamma = 1.0
        self.aov_frame = RtFrameDesc.from_buffer_copy(self.frame)
        self.aov_frame.ns = min(frame.ns, 16)
        self.reset()

    def reset(self) -> None:
        """Forget the history: the next push is a first frame."""
        self._prev = None
        self.length = None

    def push(self, camera: RtCamera, recalibrate: bool = False, spheres=None, indices=None, first: int = 0, instances=None,
             instance_indices=None, instance_first: int = 0, quads=None, quad_indices=None, quad_first: int = 0) -> np.ndarray:
        records, instance_records, quad_records = None, None, None
        if not self.follow_instances and (instances is not None or instance_indices is not None or instance_first != 0):
            raise ValueError("instances, instance_indices and instance_first need follow_instances=True")
        if not self.follow_quads and (quads is not None or quad_indices is not None or quad_first != 0):
            raise ValueError("quads, quad_indices and quad_first need follow_quads=True")
        if not self.follow_spheres and (spheres is not None or indices is not None or first != 0):
            raise ValueError("spheres, indices and first need follow_spheres=True")
        if self.follow_instances:
            if instances is not None:
                self.scene.update_instances(instances, instance_indices, instance_first)
            instance_records = self.scene.instances()
        if self.follow_quads:
            if quads is not None:
                self.scene.update_quads(quads, quad_indices, quad_first)
            quad_records = self.scene.quads()
            if instance_records is None:
                instance_records = self.scene.instances()
        if self.follow_spheres:
            if spheres is not None:
                self.scene.update_spheres(spheres, indices, first)
            records = self.scene.spheres()
        self.scene.set_camera(camera, recalibrate)
        color, _ = self.scene.render(self.frame)
        aov = self.scene.render_aov(self.aov_frame, albedo=self.denoise, ids=True)
        cam = RtCamera.from_buffer_copy(camera)
        p = self._prev
        if p is None:
            r = reproject(color, aov["depth"], aov["alpha"], cam, cam, **self.params)
        else:
            follow = {}
            if records is not None:
                follow = dict(spheres=records, prev_spheres=p["spheres"], media=self.scene.host.media())
            if instance_records is not None:
                follow.update(instances=instance_records, prev_instances=p["instances"], inst=aov["inst"], prev_inst=p["inst"],
                              media=self.scene.host.media())
            if quad_records is not None:
                follow.update(quads=quad_records, prev_quads=p["quads"])
            r = reproject(color, aov["depth"], aov["alpha"], cam, p["camera"], aov["normal"], aov["prim"], p["out"], p["length"],
                          p["depth"], p["alpha"], p["normal"], p["prim"], **self.params, **follow)
        self._prev = {"camera": cam, "out": r.out, "length": r.length, "depth": aov["depth"], "alpha": aov["alpha"],
                      "normal": aov["normal"], "prim": aov["prim"], "spheres": records, "instances": instance_records, "inst": aov["inst"],
                      "quads": quad_records}
        self.length = r.length
        if self.denoise:
            return denoise(r.out, aov["albedo"], aov["normal"], aov["depth"])
        return r.out


class MultiScene:
    """rt_multi*: one replica of the scene per GPU, driven from this thread (rt_multi_* of include/rt_abi.h)."""

    def __init__(self, host_scene: HostScene, n_gpus: int):
        global _initialised_device
        _check(rt_lib().rt_init_devices(n_gpus), "rt_init_devices")
        _initialised_device = 0
        self.host = host_scene
        self._p = C.c_void_p()
        _check(rt_lib().rt_multi_create(C.byref(host_scene.desc), n_gpus, C.byref(self._p)), "rt_multi_create")

    def set_camera(self, camera: RtCamera, recalibrate: bool = False) -> None:
        """DeviceScene.set_camera on every replica (rt_multi_set_camera)."""
        _status(rt_lib().rt_multi_set_camera(self._p, C.byref(camera), 1 if recalibrate else 0), "rt_multi_set_camera")

    def update_spheres(self, spheres, indices=None, first: int = 0, recalibrate: bool = False) -> None:
        """DeviceScene.update_spheres with host records on every replica (rt_multi_update_spheres)."""
        self._update_records(_SPHERES, "rt_multi_update_spheres", spheres, indices, first, recalibrate)

    def update_instances(self, instances, indices=None, first: int = 0, recalibrate: bool = False) -> None:
        """DeviceScene.update_instances with host records on every replica (rt_multi_update_instances)."""
        self._update_records(_INSTANCES, "rt_multi_update_instances", instances, indices, first, recalibrate)

    def update_quads(self, quads, indices=None, first: int = 0, recalibrate: bool = False) -> None:
        """DeviceScene.update_quads with host records on every replica (rt_multi_update_quads)."""
        self._update_records(_QUADS, "rt_multi_update_quads", quads, indices, first, recalibrate)

    def _update_records(self, kind, entry, records, indices, first, recalibrate):
        u, _ = _record_update(kind, records, indices, first)
        _status(getattr(rt_lib(), entry)(self._p, C.byref(u), 1 if recalibrate else 0), entry)

    def render(self, frame: RtFrameDesc, tile_rows: int = 4):
        """The whole frame as float32[ny][nx][3] in host memory, and the summed statistics."""
        out = np.empty((frame.ny, frame.nx, 3), np.float32)
        stats = RtStats()
        _check(rt_lib().rt_multi_render(self._p, C.byref(frame), out.ctypes.data, 0, tile_rows, C.byref(stats)), "rt_multi_render")
        return out, stats

    def close(self):
        if self._p:
            rt_lib().rt_multi_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_walk_array(nodes: np.ndarray, passes=None, root_visits: float = 0.0):
    """The walk array rt_scene_create would derive from `nodes` (NODE_DTYPE) for the given per-node pass counts (None = by
    surface area).  Host only.  Returns (walk nodes, tests per ray before, after)."""
    nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
    n = len(nodes)
    out = np.zeros(n, NODE_DTYPE)
    n_out, tb, ta = C.c_int32(0), C.c_double(0), C.c_double(0)
    p = None if passes is None else np.ascontiguousarray(passes, np.float64)
    _check(rt_lib().rt_plan_walk_array(nodes.ctypes.data, n, None if p is None else p.ctypes.data, float(root_visits), out.ctypes.data, n,
                                       C.byref(n_out), C.byref(tb), C.byref(ta)), "rt_plan_walk_array")
    return out[: n_out.value].copy(), tb.value, ta.value


def regroup_leaves(nodes: np.ndarray, method: int = 0) -> np.ndarray:
    """The leaves of `nodes` (NODE_DTYPE) under another binary tree over the same leaf order (method 0 = top-down by
    surface-area cost, 1 = bottom-up).  Host only."""
    nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
    out = np.zeros(2 * len(nodes), NODE_DTYPE)
    n_out = C.c_int32(0)
    _check(rt_lib().rt_regroup_leaves(nodes.ctypes.data, len(nodes), int(method), out.ctypes.data, len(out), C.byref(n_out)), "rt_regroup_leaves")
    return out[: n_out.value].copy()


def row_owner(global_row: int, tile_rows: int, n_gpus: int):
    d, l = C.c_int32(0), C.c_int32(0)
    _check(rt_lib().rt_multi_row_owner(global_row, tile_rows, n_gpus, C.byref(d), C.byref(l)), "rt_multi_row_owner")
    return d.value, l.value


def local_rows_to_global(frame: RtFrameDesc) -> np.ndarray:
    L = rt_lib()
    rows = L.rt_frame_local_rows(C.byref(frame))
    return np.array([L.rt_local_to_global_row(C.byref(frame), k) for k in range(rows)], np.int64)


def write_ppm(path: str, fb: np.ndarray, double_scale: bool = False, binary: bool = False) -> None:
    """ASCII P3 as the reference prints it (main.cu:715-727, unclamped), or binary P6 (clamped to 0..255)."""
    fb = np.ascontiguousarray(fb, np.float32)
    ny, nx = fb.shape[0], fb.shape[1]
    if host_lib().rtw_write_ppm(path.encode(), fb.ctypes.data, nx, ny, (1 if double_scale else 0) | (2 if binary else 0)) != 0:
        raise RtError(f"cannot write {path}")
