#!/usr/bin/env python3
"""rt_render_variance and rt_denoise_variance on an MI355X.

Every time is the median of 10 calls between device events, device buffers, nothing allocated inside the window.
  render   rt_render_variance against rt_render at the same ns, from the same process: the random-spheres scene at 1200 x 800 and
           the Cornell box at 600 x 600, ns = 4, 16, 64, B = min(ns, 16).  The variance passes have no cost-aware schedule, so
           the ratio is expected above 1 and growing with ns; it is recorded as measured.
  denoise  rt_denoise_variance against rt_denoise with the shipped colour factor at 1200 x 800, K = 5, every guide, beside the
           device-to-device copy that tools/bench_denoise.py times with guides: a copy of 24 B per pixel, i.e. 24 B read + 24 B
           written -- the same 48 B an iteration must move at the least (32 B read + 16 B written), in another split.
One JSON line per measurement goes to stdout and, with --out, is appended to that file (profiles/variance_mi355x.jsonl).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import accelerated_ray_tracer_amd as art  # noqa: E402


def median_ms(fn, calls=10, warmup=2):
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["render", "denoise"], default=None)
    ap.add_argument("--ns", type=int, nargs="*", default=[4, 16, 64])
    args = ap.parse_args()
    art.init(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    if args.only in (None, "render"):
        for scene, nx, ny in (("bouncing", 1200, 800), ("cornell", 600, 600)):
            hs = art.HostScene(scene, nx, ny)
            ds = art.DeviceScene(hs)
            fb = torch.empty((ny, nx, 3), dtype=torch.float32, device=dev)
            var = torch.empty((ny, nx), dtype=torch.float32, device=dev)
            for ns in args.ns:
                B = min(ns, 16)
                frame = hs.frame(ns=ns, gamma=1.0)
                plain = median_ms(lambda: ds.render(frame, out=fb.data_ptr(), stream=stream.cuda_stream, blocking=False) and ds.finish())
                st = []
                with_var = median_ms(lambda: st.append(ds.render_variance(frame, B, out=fb, variance_out=var, stream=stream.cuda_stream)[2]))
                emit({"what": "rt_render_variance", "scene": scene, "nx": nx, "ny": ny, "ns": ns, "batches": B,
                      "render_ms": round(plain, 3), "render_variance_ms": round(with_var, 3), "ratio": round(with_var / plain, 3),
                      "device_ms_render_variance": round(statistics.median(s.ms_render for s in st[-10:]), 3)})
            ds.close()

    if args.only in (None, "denoise"):
        nx, ny, K = 1200, 800, 5
        hs = art.HostScene("bouncing", nx, ny)
        ds = art.DeviceScene(hs)
        frame = hs.frame(ns=4, gamma=1.0)
        noisy, variance, _ = ds.render_variance(frame, 4)
        aov = ds.render_aov(frame, alpha=False)
        t = {k: torch.from_numpy(v).to(dev) for k, v in dict(aov, color=noisy, variance=variance).items()}
        out = torch.empty_like(t["color"])
        vout = torch.empty_like(t["variance"])
        ws = torch.empty(art.denoise_workspace_bytes(nx, ny), dtype=torch.uint8, device=dev)
        src = torch.empty(nx * ny * 24, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy_ms = median_ms(lambda: dst.copy_(src))
        common = dict(out=out, workspace=ws, stream=stream.cuda_stream, blocking=False, iterations=K)
        for lds in (-1, 0, 1):
            art.set_option("denoise_lds", lds)
            colour = median_ms(lambda: art.denoise(t["color"], t["albedo"], t["normal"], t["depth"], **common))
            guided = median_ms(lambda: art.denoise(t["color"], t["albedo"], t["normal"], t["depth"], variance=t["variance"], **common))
            guided_out = median_ms(lambda: art.denoise(t["color"], t["albedo"], t["normal"], t["depth"], variance=t["variance"], variance_out=vout,
                                                       **common))
            emit({"what": "rt_denoise_variance", "denoise_lds": lds, "nx": nx, "ny": ny, "iterations": K, "denoise_colour_factor_ms": round(colour, 4),
                  "denoise_variance_ms": round(guided, 4), "denoise_variance_with_variance_out_ms": round(guided_out, 4),
                  "ratio": round(guided / colour, 3), "copy_ms": round(copy_ms, 4), "copy_bytes_per_pixel_moved": 48,
                  "mean_iteration_over_copy": round(guided / K / copy_ms, 2)})
        art.reset_options()
        ds.close()

    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
