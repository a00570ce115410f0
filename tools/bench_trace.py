#!/usr/bin/env python3
"""Throughput of the batched ray queries (rt_trace_rays through DeviceScene.trace) on one GPU.

Ray sets, per scene (bouncing: spheres-only family; final: general family, media):
  coherent    pixel-centre primary rays of a 1200x800 frame from the scene's rt_camera (no lens offset, time0)
  incoherent  every ray of an oracle render of the scene at 300x200 @ 8 spp (orc_ray_sample: primary rays and every
              bounce), tiled to about 16 M rays
For each set, query mode (closest / any) and trace_lds (0 = scene through L1/L2, -1 = auto, and the forced LDS modes):
warm-up calls, then two timings of --reps calls each, the median reported, and a check that every call returned the same
outputs.  One JSON line per configuration on stdout.
  ms_kernel  torch events around one call enqueued behind a sleep kernel on the same stream: the host work of the call
             (argument and pointer checks, occupancy query, output allocation) is done while the GPU is still asleep, so
             the events bracket the trace kernel alone (plus one launch gap).  grays_per_s is computed from this.
  ms_call    torch events around one call on an idle stream: what a caller that waits for each call sees, host work included.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import accelerated_ray_tracer_amd as art   # noqa: E402
import oracle   # noqa: E402  (the incoherent ray sets)


def coherent_rays(hs, nx=1200, ny=800):
    c = hs.desc.camera
    i, j = np.meshgrid(np.arange(nx, dtype=np.float32), np.arange(ny, dtype=np.float32))
    u = ((i + 0.5) / nx).reshape(-1, 1)
    v = ((j + 0.5) / ny).reshape(-1, 1)
    org = np.array(c.origin, np.float32)
    d = np.array(c.lower_left_corner, np.float32) + u * np.array(c.horizontal, np.float32) + v * np.array(c.vertical, np.float32) - org
    o = np.broadcast_to(org, d.shape)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), np.full(len(d), np.float32(c.time0))


def incoherent_rays(name, target):
    img, iw, ih = art.default_texture(name)
    o = oracle.OracleScene(name, 300, 200, img, iw, ih)
    L = oracle.lib()
    L.orc_ray_sample.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_void_p, C.c_int]
    cap = 300 * 200 * 8 * 50
    rays = np.zeros((cap, 8), np.float32)
    m = L.orc_ray_sample(o.h, 300, 200, 8, 0, 200, 1, rays.ctypes.data, cap)
    rays = np.concatenate([rays[:m]] * max(1, round(target / m)))
    return np.ascontiguousarray(rays[:, 0:3]), np.ascontiguousarray(rays[:, 3:6]), np.ascontiguousarray(rays[:, 6]), m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="bouncing,final")
    ap.add_argument("--rays", type=float, default=16e6, help="size of the incoherent sets")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lds", default="0,1,2,-1")
    ap.add_argument("--sleep-cycles", type=int, default=5_000_000, help="length of the sleep kernel the kernel timing starts behind")
    a = ap.parse_args()
    import torch
    art.init(0)
    for name in a.scenes.split(","):
        img, iw, ih = art.default_texture(name)
        hs = art.HostScene(name, 1200, 800, img, iw, ih)
        ds = art.DeviceScene(hs)
        sets = {"coherent": coherent_rays(hs) + (None,), "incoherent": incoherent_rays(name, a.rays)}
        for set_name, (o, d, tm, sampled) in sets.items():
            ot, dt, tt = (torch.from_numpy(x).cuda() for x in (o, d, tm))
            n = len(o)
            for mode in ("closest", "any"):
                for lds in (int(x) for x in a.lds.split(",")):
                    art.set_option("trace_lds", lds)
                    call = lambda: ds.trace(ot, dt, tt, any_hit=(mode == "any"))   # noqa: E731
                    first = call()
                    for _ in range(a.warmup):
                        call()
                    same = True

                    def timed(blocker):
                        nonlocal same
                        times = []
                        for _ in range(a.reps):
                            torch.cuda.synchronize()
                            if blocker:
                                torch.cuda._sleep(a.sleep_cycles)
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            r = call()
                            e1.record()
                            e1.synchronize()
                            times.append(e0.elapsed_time(e1))
                            if mode == "any":
                                same = same and torch.equal(r, first)
                            else:
                                same = same and torch.equal(r.t.view(torch.int32), first.t.view(torch.int32)) and torch.equal(r.prim, first.prim)
                        return times
                    kernel, whole = timed(True), timed(False)
                    art.reset_options()
                    ms, ms_call = float(np.median(kernel)), float(np.median(whole))
                    hit = float((first if mode == "any" else first.prim >= 0).float().mean())
                    print(json.dumps({"scene": name, "rays": set_name, "n": n, "sampled_rays": sampled, "mode": mode, "trace_lds": lds,
                                      "ms_kernel": round(ms, 4), "ms_kernel_min": round(min(kernel), 4), "ms_kernel_max": round(max(kernel), 4),
                                      "ms_call": round(ms_call, 4), "grays_per_s": round(n / ms / 1e6, 3),
                                      "grays_per_s_call": round(n / ms_call / 1e6, 3), "hit_fraction": round(hit, 4),
                                      "outputs_identical": bool(same)}),
                          flush=True)
                    if not same:
                        raise SystemExit("repeated calls returned different outputs")
        ds.close()


if __name__ == "__main__":
    main()
