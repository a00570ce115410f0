#!/usr/bin/env python3
"""rt_denoise on an MI355X: 1200 x 800 at K = 5, with every guide (albedo, normal, depth, colour) and with none.

Input: the `bouncing` scene's 4-spp frame at gamma 1 and its feature buffers, on the device.  Every time is the median of
10 calls between device events (device tensors, a caller's workspace, nothing allocated or copied inside the window).  Per
configuration: the total, and the time of iteration k as (K = k + 1) - (K = k) with the pack pass in K = 0 ... i.e. the
differences of the totals at K = 1..5.  Two yardsticks from the same process:
  copy    a device-to-device copy that moves what one iteration must move at the least -- 32 B read + 16 B written per pixel
          with guides (a copy of 24 B per pixel: 24 read + 24 written), 16 + 16 without (a copy of 16 B per pixel);
  render  rt_render of the same frame at 4 spp.
One JSON line per configuration goes to stdout and, with --out, is appended to that file (profiles/denoise_bench_mi355x.jsonl).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import accelerated_ray_tracer_amd as art  # noqa: E402


def median_ms(fn, calls=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=800)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nx, ny, K = args.nx, args.ny, args.iterations
    art.init(0)
    dev = torch.device("cuda", 0)
    hs = art.HostScene("bouncing", nx, ny)
    ds = art.DeviceScene(hs)
    frame = hs.frame(ns=4, gamma=1.0)
    noisy, _ = ds.render(frame)
    aov = ds.render_aov(frame, alpha=False)
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(aov, color=noisy).items()}
    out = torch.empty_like(t["color"])
    ws = torch.empty(art.denoise_workspace_bytes(nx, ny), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    fb = torch.empty_like(t["color"])
    render_ms = median_ms(lambda: ds.render(frame, out=fb.data_ptr(), stream=stream.cuda_stream, blocking=False) and ds.finish())
    lines = []
    for name, guides, params in (("all_guides", ("albedo", "normal", "depth"), art.DENOISE_DEFAULTS),
                                 ("no_guides", (), dict(art.DENOISE_DEFAULTS, sigma_color=0.0))):
        per_pixel = 24 if guides else 16
        src = torch.empty(nx * ny * per_pixel, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy_ms = median_ms(lambda: dst.copy_(src))
        for lds in (-1, 0, 1):
            art.set_option("denoise_lds", lds)
            totals = []
            for k in range(1, K + 1):
                kw = dict(params, iterations=k)
                totals.append(median_ms(lambda: art.denoise(t["color"], *(t[g] for g in guides), out=out, workspace=ws, stream=stream.cuda_stream,
                                                            blocking=False, **kw) if len(guides) == 3 else
                                        art.denoise(t["color"], out=out, workspace=ws, stream=stream.cuda_stream, blocking=False, **kw)))
            per_iter = [totals[0]] + [totals[k] - totals[k - 1] for k in range(1, K)]
            lines.append({"what": "rt_denoise", "config": name, "denoise_lds": lds, "nx": nx, "ny": ny, "iterations": K,
                          "total_ms": round(totals[-1], 4), "totals_ms_K1_to_K": [round(x, 4) for x in totals],
                          "iteration_ms_first_includes_pack": [round(x, 4) for x in per_iter],
                          "copy_ms": round(copy_ms, 4), "copy_bytes_per_pixel_moved": 2 * per_pixel, "render_4spp_ms": round(render_ms, 4),
                          "mean_iteration_over_copy": round(totals[-1] / K / copy_ms, 2), "total_over_render_4spp": round(totals[-1] / render_ms, 3)})
        art.reset_options()
    ds.close()
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
