#!/usr/bin/env python3
"""Time of the feature pass (rt_render_aov through DeviceScene.render_aov) on one GPU, beside the two ways a caller had before.

Per scene (book1: spheres-only family; final: general family, media, every texture kind) at 1200x800, for ns in --ns and
aov_lds in --lds: the full output set (albedo, normal, depth, alpha, prim, inst, mat) and depth alone, into torch tensors.
Warm-up calls, then --reps calls, the median reported, and a check that every call returned the same outputs.  In the same
process:
  twin_render  rt_render of the emissive twin (tests/aov_expect.py) at the same frame, ns and gamma 1: the only way to an
               albedo buffer without the pass, on the render path as it is.  Its frame must equal the pass's albedo.
  trace        rt_trace_rays, closest hit, on the pass's ns = 1 primary rays (the oracle's ray sample of the twin): the
               rate of one-ray-per-lane queries on the same rays, read from a row-major list instead of 8 x 8 blocks.
One JSON line per configuration on stdout.
  ms_kernel  torch events around one call enqueued behind a sleep kernel on the same stream (tools/bench_trace.py): the host
             work of the call is done while the GPU is still asleep, so the events bracket the kernel alone.
             grays_per_s = nx * ny * ns primary rays over this.
  ms_call    torch events around one blocking call on an idle stream, host work included.
  ms_render  rt_render's own device time (rt_stats.ms_render).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import accelerated_ray_tracer_amd as art   # noqa: E402
import oracle   # noqa: E402  (the primary rays of the trace leg)
import aov_expect as ax   # noqa: E402
import trace_families as tf   # noqa: E402

NX, NY = 1200, 800


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="book1,final")
    ap.add_argument("--ns", default="1,16")
    ap.add_argument("--lds", default="-1,0")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sleep-cycles", type=int, default=5_000_000)
    a = ap.parse_args()
    import torch
    art.init(0)
    dev = torch.device("cuda", 0)

    def timed(call, blocker):
        out = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            if blocker:
                torch.cuda._sleep(a.sleep_cycles)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    def line(**kw):
        print(json.dumps(kw), flush=True)

    for name in a.scenes.split(","):
        img, iw, ih = art.default_texture(name)
        hs = art.HostScene(name, NX, NY, img, iw, ih)
        twin = ax.Twin(art, hs)
        ds, lit = art.DeviceScene(hs), art.DeviceScene(twin)
        stream = torch.cuda.current_stream(dev).cuda_stream
        shapes = {k: (NY, NX, 3) if ch == 3 else (NY, NX) for k, (ch, _) in art.AOV_OUTPUTS.items()}
        full = {k: torch.zeros(shapes[k], dtype=torch.float32 if t == np.float32 else torch.int32, device=dev)
                for k, (_, t) in art.AOV_OUTPUTS.items()}
        fb = torch.zeros((NY, NX, 3), dtype=torch.float32, device=dev)

        # rt_trace_rays on the ns = 1 primary rays
        lit_orc = oracle.OracleScene.from_desc(twin.desc, NX, NY, 1.0, hs.background, hs.use_gradient_bg)
        rays = tf.ray_sample(oracle, lit_orc, NX, NY, 1)
        assert len(rays) == NX * NY
        ot, dt, tt = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rays[:, 0:3], rays[:, 3:6], rays[:, 6]))
        first = ds.trace(ot, dt, tt)
        for _ in range(a.warmup):
            ds.trace(ot, dt, tt)
        kernel = timed(lambda: ds.trace(ot, dt, tt), True)
        ms = float(np.median(kernel))
        trace_rate = NX * NY / ms / 1e6
        line(what="trace", scene=name, n=NX * NY, ms_kernel=round(ms, 4), ms_kernel_min=round(min(kernel), 4),
             ms_kernel_max=round(max(kernel), 4), grays_per_s=round(trace_rate, 3))

        for ns in (int(x) for x in a.ns.split(",")):
            frame = hs.frame(nx=NX, ny=NY, ns=ns, gamma=1.0)
            times = []
            for k in range(a.warmup + a.reps):
                _, st = lit.render(frame, out=fb.data_ptr())
                if k >= a.warmup:
                    times.append(st.ms_render)
            ms_twin = float(np.median(times))
            line(what="twin_render", scene=name, nx=NX, ny=NY, ns=ns, rays=int(st.rays), ms_render=round(ms_twin, 4),
                 ms_render_min=round(min(times), 4), ms_render_max=round(max(times), 4), grays_per_s=round(NX * NY * ns / ms_twin / 1e6, 3))
            for lds in (int(x) for x in a.lds.split(",")):
                for outputs in ("all", "depth"):
                    out = full if outputs == "all" else {"depth": full["depth"]}
                    art.set_option("aov_lds", lds)
                    call = lambda: ds.render_aov(frame, out=out, stream=stream, blocking=False)   # noqa: E731
                    call()
                    torch.cuda.synchronize()
                    keep = {k: v.clone() for k, v in out.items()}
                    for _ in range(a.warmup):
                        call()
                    kernel = timed(call, True)
                    whole = timed(lambda: ds.render_aov(frame, out=out, stream=stream), False)
                    art.reset_options()
                    torch.cuda.synchronize()
                    same = all(torch.equal(out[k].view(torch.int32), keep[k].view(torch.int32)) for k in out)
                    ms, ms_call = float(np.median(kernel)), float(np.median(whole))
                    rec = dict(what="aov", scene=name, nx=NX, ny=NY, ns=ns, aov_lds=lds, outputs=outputs, ms_kernel=round(ms, 4),
                               ms_kernel_min=round(min(kernel), 4), ms_kernel_max=round(max(kernel), 4), ms_call=round(ms_call, 4),
                               grays_per_s=round(NX * NY * ns / ms / 1e6, 3), time_over_twin_render=round(ms / ms_twin, 3),
                               rate_over_trace=round(NX * NY * ns / ms / 1e6 / trace_rate, 3), outputs_identical=bool(same))
                    if outputs == "all":
                        rec["albedo_equals_twin_render"] = bool(torch.equal(full["albedo"].view(torch.int32), fb.view(torch.int32)))
                        if ns == 1:
                            hit = first.prim >= 0
                            rec["depth_equals_trace"] = bool(torch.equal(full["depth"].reshape(-1)[hit].view(torch.int32), first.t[hit].view(torch.int32)))
                    line(**rec)
                    if not same:
                        raise SystemExit("repeated calls returned different outputs")
        ds.close()
        lit.close()


if __name__ == "__main__":
    main()
