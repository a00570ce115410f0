#!/usr/bin/env python3
"""Throughput of the radiance queries (rt_radiance_rays through DeviceScene.radiance) on one GPU, beside rt_render.

Per scene (bouncing: spheres-only family; final: general family, media, every texture kind): the pixel-centre primary rays of
a 1200x800 frame from the scene's rt_camera (no lens offset, time0), one query each, for ns in --ns, radiance_lds in --lds
and with / without rays_out.  Warm-up calls, then --reps calls timed twice, the medians reported, and a check that every call
returned the same outputs.  One JSON line per configuration on stdout.
  ms_kernel  torch events around one call enqueued behind a sleep kernel on the same stream (tools/bench_trace.py): the
             host work of the call is done while the GPU is still asleep, so the events bracket the kernel alone.
             grays_per_s = the batch's world->hit calls (the sum of rays_out) over this.
  ms_call    torch events around one call on an idle stream, host work included.
Beside each (scene, ns): rt_render of the same scene at 1200x800 and the same ns from this process ("render" lines: the
median device time of --reps frames and its rays / s).  The two do not trace the same rays -- a render jitters its samples
inside the pixel and through the lens -- so the comparison is of rates, not of times.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import accelerated_ray_tracer_amd as art   # noqa: E402
from bench_trace import coherent_rays   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="bouncing,final")
    ap.add_argument("--ns", default="1,16")
    ap.add_argument("--lds", default="-1,0")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sleep-cycles", type=int, default=5_000_000)
    a = ap.parse_args()
    import torch
    art.init(0)
    for name in a.scenes.split(","):
        img, iw, ih = art.default_texture(name)
        hs = art.HostScene(name, 1200, 800, img, iw, ih)
        ds = art.DeviceScene(hs)
        o, d, tm = coherent_rays(hs)
        ot, dt, tt = (torch.from_numpy(x).cuda() for x in (o, d, tm))
        n = len(o)
        buf = torch.zeros((800, 1200, 3), dtype=torch.float32, device="cuda")
        for ns in (int(x) for x in a.ns.split(",")):
            frame = hs.frame(nx=1200, ny=800, ns=ns)
            times, rays = [], 0
            for k in range(a.warmup + a.reps):
                _, st = ds.render(frame, out=buf.data_ptr())
                if k >= a.warmup:
                    times.append(st.ms_render)
                rays = int(st.rays)
            ms = float(np.median(times))
            print(json.dumps({"what": "render", "scene": name, "nx": 1200, "ny": 800, "ns": ns, "rays": rays, "ms_render": round(ms, 4),
                              "ms_render_min": round(min(times), 4), "ms_render_max": round(max(times), 4),
                              "grays_per_s": round(rays / ms / 1e6, 3)}), flush=True)
            render_rate = rays / ms / 1e6
            for lds in (int(x) for x in a.lds.split(",")):
                total = None
                for count in (True, False):
                    art.set_option("radiance_lds", lds)
                    call = lambda: ds.radiance(ot, dt, tt, ns=ns, count_rays=count)   # noqa: E731
                    first = call()
                    for _ in range(a.warmup):
                        call()
                    same = True

                    def timed(blocker):
                        nonlocal same
                        out = []
                        for _ in range(a.reps):
                            torch.cuda.synchronize()
                            if blocker:
                                torch.cuda._sleep(a.sleep_cycles)
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            r = call()
                            e1.record()
                            e1.synchronize()
                            out.append(e0.elapsed_time(e1))
                            same = same and torch.equal(r.rgb.view(torch.int32), first.rgb.view(torch.int32))
                            if count:
                                same = same and torch.equal(r.rays, first.rays)
                        return out
                    kernel, whole = timed(True), timed(False)
                    art.reset_options()
                    if count:
                        total = int(first.rays.sum(dtype=torch.int64))
                    ms, ms_call = float(np.median(kernel)), float(np.median(whole))
                    print(json.dumps({"what": "radiance", "scene": name, "n": n, "ns": ns, "radiance_lds": lds, "rays_out": count, "rays": total,
                                      "ms_kernel": round(ms, 4), "ms_kernel_min": round(min(kernel), 4), "ms_kernel_max": round(max(kernel), 4),
                                      "ms_call": round(ms_call, 4), "grays_per_s": round(total / ms / 1e6, 3),
                                      "rate_over_render": round(total / ms / 1e6 / render_rate, 3), "outputs_identical": bool(same)}),
                          flush=True)
                    if not same:
                        raise SystemExit("repeated calls returned different outputs")
        ds.close()


if __name__ == "__main__":
    main()
