#!/usr/bin/env python3
"""What the guided upscaler buys at equal path cost, and what it costs, on an MI355X (profiles/upscale_quality.json).

Per scene at its BASELINE size (cornell 600 x 600, bouncing 1200 x 800, final 800 x 800), against the full-resolution
rt_render at --ref-ns samples (at least 16 n) and seeds of its own, RMSE of the linear image over the whole frame (and,
beside it, the number of pixels off by more than 1 and the RMSE of the others: a few pixels can carry the whole figure):
  A  render_denoised at n samples (--ns): the full frame traced and filtered;
  B  render_upscaled at factor 2 and 4 with ns = n factor^2 -- the same number of paths as A, on a coarse grid -- with and
     without the denoiser on the coarse frame;
  C  B's coarse frame replicated pixel by pixel (what a caller without rt_upscale can do with it);
  and B's undenoised coarse frame upscaled with demodulate=False, beside the largest demodulated coarse value.
Also the share of the pixels that took the guided branch (weight_out >= min_weight and > 0).

Then the device time of rt_upscale alone (device tensors, both values of option "upscale_lds", factors 2 and 4) beside one
rt_denoise iteration on the same full frame: each figure is the median of --repeats windows of --calls calls between device
events after a warm-up, with the smallest and the largest window beside it.  A window holds the host's enqueueing as well: it is
the time of a call in a stream of calls, not of the kernel.  The kernels' own times come from a profiler run of the timing part
alone (rocprofv3 --kernel-trace --stats -- tools/upscale_quality.py --skip-quality --factors F), whose kernel statistics
--kernel-stats FILE.csv --factors F --out ... then adds to the record under "kernel_time".
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the render library is loaded, as in the other tools: both bring a HIP runtime)

import accelerated_ray_tracer_amd as art  # noqa: E402

SCENES = {"cornell": (600, 600), "bouncing": (1200, 800), "final": (800, 800)}


def rmse(img, reference):
    return float(np.sqrt(((img.astype(np.float64) - reference.astype(np.float64)) ** 2).mean()))


def errors(img, reference):
    """RMSE over the whole frame; and, because a handful of pixels can carry it, how many pixels are off by more than 1 in
    some channel and the RMSE over the others."""
    d = img.astype(np.float64) - reference.astype(np.float64)
    far = (np.abs(d) > 1.0).any(axis=2)
    return {"rmse": round(rmse(img, reference), 5), "pixels_off_by_more_than_1": int(far.sum()),
            "rmse_of_the_other_pixels": round(float(np.sqrt((d[~far] ** 2).mean())), 5)}


def quality(name, n, ref_ns):
    nx, ny = SCENES[name]
    img, iw, ih = art.default_texture(name)
    hs = art.HostScene(name, nx, ny, img, iw, ih)
    ds = art.DeviceScene(hs)
    reference = ds.render(hs.frame(ns=ref_ns, gamma=1.0, seed_base=1984 + 7 * nx * ny))[0].copy()
    a = ds.render_denoised(hs.frame(ns=n))
    line = {"scene": name, "nx": nx, "ny": ny, "n": n, "reference_ns": ref_ns,
            "A_render_denoised": dict(errors(a["color"], reference), ns=n, noisy=errors(a["noisy"], reference))}
    for f in (2, 4):
        for denoise in (True, False):
            b = ds.render_upscaled(hs.frame(ns=n * f * f), f, denoise=denoise)
            replicated = np.repeat(np.repeat(b["low"], f, axis=0), f, axis=1)
            guided = (b["weight"] >= np.float32(art.UPSCALE_DEFAULTS["min_weight"])) & (b["weight"] > 0)
            line[f"B_render_upscaled_factor_{f}" + ("_denoised" if denoise else "")] = {
                "ns": n * f * f, **errors(b["color"], reference), "C_replicated": errors(replicated, reference),
                "guided_share": round(float(guided.mean()), 4)}
        # the same coarse frame without demodulation, and what demodulation made of it: x = colour / max(albedo, 2^-10) per coarse pixel
        g_lo = ds.render_aov(hs.frame(nx=nx // f, ny=ny // f, ns=min(n * f * f, 16), gamma=1.0), alpha=False)   # (b: the undenoised one)
        plain = art.upscale(b["low"], f, normal_lo=g_lo["normal"], depth_lo=g_lo["depth"], normal=b["normal"], depth=b["depth"])
        x = (b["low"] / np.maximum(g_lo["albedo"], np.float32(2.0 ** -10))).max(axis=2)
        below = g_lo["albedo"].min(axis=2) < 2.0 ** -10
        line[f"B_render_upscaled_factor_{f}_not_demodulated"] = {
            "ns": n * f * f, **errors(plain, reference), "coarse_pixels": int(x.size), "coarse_pixels_with_x_above_8": int((x > 8).sum()),
            "of_them_with_an_albedo_channel_below_the_floor": int(((x > 8) & below).sum()), "largest_x": round(float(x.max()), 2)}
    ds.close()
    hs.close()
    return line


def window_ms(fn, calls, repeats, warmup=3):
    for _ in range(warmup * calls):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return {"median_ms": round(statistics.median(times), 5), "min_ms": round(min(times), 5), "max_ms": round(max(times), 5)}


def timing(name, calls, repeats, factors):
    nx, ny = SCENES[name]
    dev = torch.device("cuda", 0)
    img, iw, ih = art.default_texture(name)
    hs = art.HostScene(name, nx, ny, img, iw, ih)
    ds = art.DeviceScene(hs)
    full = hs.frame(ns=4, gamma=1.0)
    noisy = ds.render(full)[0]
    g = ds.render_aov(full, alpha=False)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(g, color=noisy).items()}
    out = torch.empty_like(t["color"])
    ws = torch.empty(art.denoise_workspace_bytes(nx, ny), dtype=torch.uint8, device=dev)
    line = {"scene": name, "nx": nx, "ny": ny, "calls_per_window": calls, "windows": repeats}
    one = window_ms(lambda: art.denoise(t["color"], t["albedo"], t["normal"], t["depth"], iterations=1, out=out, workspace=ws, blocking=False), calls, repeats)
    two = window_ms(lambda: art.denoise(t["color"], t["albedo"], t["normal"], t["depth"], iterations=2, out=out, workspace=ws, blocking=False), calls, repeats)
    line["rt_denoise_1_iteration_with_pack"] = one
    line["rt_denoise_2_iterations_with_pack"] = two
    line["rt_denoise_one_iteration_ms"] = round(two["median_ms"] - one["median_ms"], 5)
    for f in factors:
        lo = hs.frame(nx=nx // f, ny=ny // f, ns=4, gamma=1.0)
        low = ds.render(lo)[0]
        g_lo = ds.render_aov(lo, alpha=False)
        tl = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(g_lo, color=low).items()}
        results = {}
        for lds in (1, 0, 1, 0):   # alternating, each twice: the second pass shows the spread between windows minutes apart
            art.set_option("upscale_lds", lds)
            r = window_ms(lambda: art.upscale(tl["color"], f, tl["albedo"], tl["normal"], tl["depth"], t["albedo"], t["normal"], t["depth"],
                                              out=out, blocking=False), calls, repeats)
            results.setdefault("staged" if lds else "direct", []).append(r)
            results.setdefault("frame_" + ("staged" if lds else "direct"), out.cpu().numpy().copy())
        art.reset_options()
        same = bool(np.array_equal(results.pop("frame_staged").view(np.uint32), results.pop("frame_direct").view(np.uint32)))
        line[f"rt_upscale_factor_{f}"] = dict(results, staged_equals_direct_bit_for_bit=same)
    ds.close()
    hs.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,bouncing,final")
    ap.add_argument("--ns", type=int, default=4)
    ap.add_argument("--ref-ns", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--factors", default="2,4", help="of the timing part")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a --skip-quality run: added to --out, nothing is run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.ref_ns < 16 * args.ns:
        raise SystemExit("--ref-ns must be at least 16 times --ns")
    factors = [int(f) for f in args.factors.split(",")]
    if args.kernel_stats:
        import csv
        rows = {}
        with open(args.kernel_stats) as fh:
            for r in csv.DictReader(fh):
                if "rt_upscale_kernel" in r["Name"] or "rt_denoise_kernel" in r["Name"] or "rt_denoise_pack_kernel" in r["Name"]:
                    rows[r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")] = {
                        "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3), "min_us": round(float(r["MinNs"]) / 1e3, 3),
                        "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
        with open(args.out) as fh:
            result = json.load(fh)
        result.setdefault("kernel_time", {})[f"scenes_{args.scenes}_factors_{args.factors}"] = rows
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
        print(json.dumps(rows))
        return
    art.init(0)
    result = {"what": "guided upscaling against a denoised full-resolution frame at equal path cost, and the device time of rt_upscale",
              "upscale_defaults": art.UPSCALE_DEFAULTS, "quality": [], "timing": []}
    for name in [] if args.skip_quality else args.scenes.split(","):
        result["quality"].append(quality(name, args.ns, args.ref_ns))
        print(json.dumps(result["quality"][-1]), flush=True)
    for name in args.scenes.split(","):
        result["timing"].append(timing(name, args.calls, args.repeats, factors))
        print(json.dumps(result["timing"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
