#!/usr/bin/env python3
"""Launch shapes of every render entry point, one JSON line per case: what a change of the host code that plans the launches
(csrc/rt_abi.hip) must leave as it is.  A wrong grid or LDS size still renders the right frame, so the test suite does not see
it.  Per case: the launch fields of rt_stats, the 13 words of rt_debug_rank_info where the frame was ranked -- then also the number
of parts it ran as (rt_debug_cost_map) and the counts between which its tails were ordered (rt_debug_handoff_queue) --, whether
the tail hand-off took pixels, the passes of an adaptive frame, and the SHA-256 of the outputs.  The cases: 64x64-class frames
through every render entry, then whole frames and row shares of the three scene families, repeat frames (exact and stale cost
map) and one frame per option of the schedule, so that every regime of csrc/rt_frame_plan.h is reached.

  RT_LIB_OVERRIDE=<library of the parent commit> python tools/launch_shapes.py > parent.jsonl
  python tools/launch_shapes.py > new.jsonl && diff parent.jsonl new.jsonl

RT_OPTS=key=value,... sets knobs for the whole run: with cost_map=0 (the cost map off, DESIGN.md 4.3c: the second render of a
scene is ranked like its first) the output is that of a library from before the map.

profiles/frame_plan_launch_shapes.jsonl is this tool's output on an MI355X (profiles/abi_refactor_launch_shapes.jsonl: its first
half, from before the later cases were added)."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import accelerated_ray_tracer_amd as art   # noqa: E402

art.init(0)


def shipped_options():
    art.reset_options()
    for kv in filter(None, os.environ.get("RT_OPTS", "").split(",")):
        k, v = kv.split("=")
        art.set_option(k, int(v))


shipped_options()
L = art.rt_lib()
L.rt_debug_handoff.argtypes = [C.c_void_p, C.c_void_p]


def emit(case, **kw):
    print(json.dumps(dict(case=case, **kw), sort_keys=True), flush=True)


def stats_dict(st):
    return {k: int(getattr(st, k)) for k in ("kernel_variant", "workgroups", "threads_per_group", "lds_bytes", "samples", "reserved")}


def rank_and_handoff(ds):
    w = np.zeros(13, np.uint32)
    ranked = L.rt_debug_rank_info(ds._p, w.ctypes.data) == 0
    h = np.zeros(2, np.uint64)
    assert L.rt_debug_handoff(ds._p, h.ctypes.data) == 0
    out = dict(rank_info=[int(x) for x in w] if ranked else None, handoff=[bool(h[0]), bool(h[1])])
    if ranked:   # the schedule's own words: how many parts the frame ran as, and between which counts its tails were ordered
        out["parts"] = ds.cost_map()[2]
        out["tail_order"] = ds.handoff_queue()[3]
    return out


def sha(*arrays):
    m = hashlib.sha256()
    for a in arrays:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def dev_buf(n, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype, device="cuda:0")


for scene in ("random_scene", "cornell"):
    frames = [("64x64@32", dict(nx=64, ny=64, ns=32)), ("64x64@8", dict(nx=64, ny=64, ns=8)),
              ("64x64@32 share", dict(nx=64, ny=64, ns=32, tile_rows=8, tile_stride=2, tile_first=1)),
              ("61x43@32", dict(nx=61, ny=43, ns=32)), ("131x67@32", dict(nx=131, ny=67, ns=32))]
    for name, kw in frames:
        hs = art.HostScene(scene, kw["nx"], kw["ny"])
        ds = art.DeviceScene(hs)
        f = hs.frame(**kw)
        rows = L.rt_frame_local_rows(C.byref(f))
        for where in ("host", "device"):
            if where == "host":
                fb, st = ds.render(f)
                digest = sha(fb)
            else:
                t = dev_buf(rows * f.nx * 3)
                _, st = ds.render(f, out=t.data_ptr())
                digest = sha(t.cpu().numpy())
            emit(f"{scene} rt_render {name} {where} fb", fb_sha256=digest, **stats_dict(st), **rank_and_handoff(ds))
        ds.close()

    hs = art.HostScene(scene, 64, 64)
    ds = art.DeviceScene(hs)
    f = hs.frame(nx=64, ny=64, ns=16)
    pf = ds.progressive(f)
    for b, e in ((0, 8), (8, 16)):
        fb, st = pf.render(b, e)
        emit(f"{scene} rt_render_window [{b},{e})", fb_sha256=sha(fb), **stats_dict(st), **rank_and_handoff(ds))
    pf.close()

    for tier in (0, 1):
        art.set_option("adaptive_tier", tier)
        for where in ("host", "device"):
            fa = hs.frame(nx=64, ny=64, ns=32)
            if where == "host":
                fb, spp, st = ds.render_adaptive(fa, 4, 32, 0.05)
                digest = sha(fb, spp)
            else:
                t, ts = dev_buf(64 * 64 * 3), dev_buf(64 * 64, torch.int32)
                _, _, st = ds.render_adaptive(fa, 4, 32, 0.05, out=t, spp_out=ts)
                digest = sha(t.cpu().numpy(), ts.cpu().numpy())
            passes = [[p["route"], p["active"], p["samples"][0], p["samples"][1]] for p in ds.adaptive_passes()]
            emit(f"{scene} rt_render_adaptive 4..32 adaptive_tier={tier} {where} fb", fb_sha256=digest, passes=passes, **stats_dict(st))
    shipped_options()

    for where in ("host", "device"):
        fv = hs.frame(nx=64, ny=64, ns=16)
        if where == "host":
            fb, var, st = ds.render_variance(fv, 4)
            digest = sha(fb, var)
        else:
            t, tv = dev_buf(64 * 64 * 3), dev_buf(64 * 64)
            _, _, st = ds.render_variance(fv, 4, out=t, variance_out=tv)
            digest = sha(t.cpu().numpy(), tv.cpu().numpy())
        emit(f"{scene} rt_render_variance 4x4 {where} fb", fb_sha256=digest, **stats_dict(st))

    fq = hs.frame(nx=64, ny=64, ns=4)
    aov = ds.render_aov(fq, ids=True)
    emit(f"{scene} rt_render_aov host", sha256=sha(*[aov[k] for k in sorted(aov)]))
    thr = ds.render_aov_through(fq, ids=True, through=True, bounces=True)
    emit(f"{scene} rt_render_aov_through host", sha256=sha(*[thr[k] for k in sorted(thr)]))
    noisy, _ = ds.render(fq)
    noisy = np.ascontiguousarray(noisy.reshape(64, 64, 3))
    den = art.denoise(noisy, albedo=np.ascontiguousarray(aov["albedo"].reshape(64, 64, 3)), normal=np.ascontiguousarray(aov["normal"].reshape(64, 64, 3)),
                      depth=np.ascontiguousarray(aov["depth"].reshape(64, 64)))
    emit(f"{scene} rt_denoise host", sha256=sha(den))
    ds.close()


# ---- the regimes the 64x64-class frames above never reach (csrc/rt_frame_plan.h): whole frames, halves, quarters and eighths on
# both sides of 2.75 / 1.375 / 0.6875 pixels per resident lane, repeat frames ranked on the cost map, and the schedule's options.
# One frame each, into device memory.
def one_frame(ds, hs, case, **kw):
    f = hs.frame(**kw)
    t = dev_buf(L.rt_frame_local_rows(C.byref(f)) * f.nx * 3)
    _, st = ds.render(f, out=t.data_ptr())
    emit(case, fb_sha256=sha(t.cpu().numpy()), **stats_dict(st), **rank_and_handoff(ds))


def shifted(cam):
    out = type(cam).from_buffer_copy(cam)
    for k, d in enumerate((0.05, 0.03, -0.04)):
        out.origin[k] += d
        out.lower_left_corner[k] += d
    return out


for scene, nx, ny in (("random_scene", 1200, 800), ("cornell", 600, 600), ("final", 800, 800)):
    hs = art.HostScene(scene, nx, ny, *art.default_texture(scene))
    ds = art.DeviceScene(hs)
    one_frame(ds, hs, f"{scene} {nx}x{ny}@32 whole", nx=nx, ny=ny, ns=32)
    if scene == "random_scene":
        one_frame(ds, hs, f"{scene} {nx}x{ny}@32 whole again (exact map)", nx=nx, ny=ny, ns=32)
        ds.set_camera(shifted(hs.desc.camera))
        one_frame(ds, hs, f"{scene} {nx}x{ny}@32 whole, camera moved (stale map)", nx=nx, ny=ny, ns=32)
    for stride in (2, 4, 8) if scene == "random_scene" else (8,):
        one_frame(ds, hs, f"{scene} {nx}x{ny}@32 rank 0 of {stride}", nx=nx, ny=ny, ns=32, tile_rows=4, tile_first=0, tile_stride=stride)
    ds.close()

hs = art.HostScene("random_scene", 256, 256)
for key, value, ns in (("prior", 0, 32), ("presplit_samples", 8, 32), ("resplit_samples", 32, 64), ("handoff_order", 0, 32), ("handoff", 0, 32),
                       ("tier_kernel", 0, 32), ("cost_map", 0, 32), ("lds_mode", 1, 32), ("wg_per_cu", 1, 32)):
    art.set_option(key, value)
    ds = art.DeviceScene(hs)
    one_frame(ds, hs, f"random_scene 256x256@{ns} {key}={value}", nx=256, ny=256, ns=ns)
    ds.close()
    shipped_options()
