"""Adaptive sampling on one GPU: time, mean spp, rays and the passes of rt_render_adaptive per configuration, against
rt_render at max_spp (the control), with the tier route forced off / on next to auto, and the quality
(RMSE against the fixed max_spp frame, and of a fixed frame at the same mean spp).  One JSON line per run.

    python tools/adaptive_sweep.py --config cornell --out profiles/adaptive_mi355x.jsonl
    python tools/adaptive_sweep.py --config random --out ...
    python tools/adaptive_sweep.py --config crossover --out ...   # the routes against the active-pixel count

The crossover configuration renders row shares (1-row tiles dealt to a world of N: nx * ny / N pixels) at threshold -1, so
that every pass has a known number of active pixels, with the route forced to the main kernel (0), the tier kernel (1) and
auto (-1); the pass times of the two forced routes set the auto crossover.

Each timed value is the best of --reps runs after one warm-up run of the same configuration.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import accelerated_ray_tracer_amd as art  # noqa: E402

CONFIGS = {
    "cornell": dict(scene="cornell", nx=600, ny=600, min_spp=16, max_spp=1024, thresholds=[0.01, 0.03, 0.1, -1.0], routes=[-1, 0, 1]),
    "random": dict(scene="bouncing", nx=1200, ny=800, min_spp=16, max_spp=512, thresholds=[0.01, 0.03, 0.1, -1.0], routes=[-1, 0, 1]),
}


CROSSOVER = dict(scenes=[("cornell", 600, 600), ("bouncing", 1200, 800)], worlds=[4, 16, 64, 256, 1024], min_spp=16, max_spp=256)


def crossover(args, emit_file):
    c = CROSSOVER
    for name, nx, ny in c["scenes"]:
        img, iw, ih = art.default_texture(name)
        hs = art.HostScene(name, nx, ny, img, iw, ih)
        ds = art.DeviceScene(hs)
        for world in c["worlds"]:
            f = hs.frame(ns=1, tile_rows=1, tile_first=0, tile_stride=world)
            for route in (0, 1, -1):
                art.set_option("adaptive_tier", route)
                ds.render_adaptive(f, c["min_spp"], c["max_spp"], -1.0, args.floor)
                best = None
                for _ in range(args.reps):
                    _, _, st = ds.render_adaptive(f, c["min_spp"], c["max_spp"], -1.0, args.floor)
                    if best is None or st.ms_render < best[0].ms_render:
                        best = (st, ds.adaptive_passes())
                st, passes = best
                rec = {"kind": "crossover", "scene": name, "nx": nx, "ny": ny, "world": world, "pixels": passes[0]["active"],
                       "adaptive_tier": route, "ms": round(st.ms_render, 3), "rays": st.rays,
                       "passes": [{"route": p["route"], "active": p["active"], "samples": p["samples"], "ms": p["ms"]} for p in passes]}
                line = json.dumps(rec)
                print(line, flush=True)
                emit_file.write(line + "\n")
                emit_file.flush()
        art.reset_options()
        ds.close()


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS) + ["crossover"], required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    art.init(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.config == "crossover":
        with open(args.out, "a") as fo:
            crossover(args, fo)
        return
    c = CONFIGS[args.config]
    img, iw, ih = art.default_texture(c["scene"])
    hs = art.HostScene(c["scene"], c["nx"], c["ny"], img, iw, ih)
    ds = art.DeviceScene(hs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(rec):
        rec.update(scene=c["scene"], nx=c["nx"], ny=c["ny"])
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def fixed(ns):
        ds.render(hs.frame(ns=ns))
        best = None
        for _ in range(args.reps):
            fb, st = ds.render(hs.frame(ns=ns))
            best = st.ms_render if best is None else min(best, st.ms_render)
        return fb, st, best

    ref, rst, rms = fixed(c["max_spp"])
    emit({"kind": "control", "ns": c["max_spp"], "ms": round(rms, 3), "rays": rst.rays, "grays_per_s": round(rst.rays / rms / 1e6, 4)})
    px = c["nx"] * c["ny"]
    for t in c["thresholds"]:
        for route in c["routes"]:
            art.set_option("adaptive_tier", route)
            ds.render_adaptive(hs.frame(ns=1), c["min_spp"], c["max_spp"], t, args.floor)
            best = None
            for _ in range(args.reps):
                fb, spp, st = ds.render_adaptive(hs.frame(ns=1), c["min_spp"], c["max_spp"], t, args.floor)
                if best is None or st.ms_render < best[2].ms_render:
                    best = (fb, spp, st, ds.adaptive_passes())
            fb, spp, st, passes = best
            mean = st.samples / px
            rec = {"kind": "adaptive", "threshold": t, "floor": args.floor, "min_spp": c["min_spp"], "max_spp": c["max_spp"],
                   "adaptive_tier": route, "ms": round(st.ms_render, 3), "mean_spp": round(mean, 3), "rays": st.rays,
                   "grays_per_s": round(st.rays / st.ms_render / 1e6, 4), "vs_control": round(st.ms_render / rms, 4),
                   "passes": [{"route": p["route"], "active": p["active"], "samples": p["samples"], "ms": p["ms"]} for p in passes],
                   "rmse_vs_max": rmse(fb, ref)}
            if route == c["routes"][0] and t >= 0:
                eq = max(1, int(round(mean)))
                efb, est, ems = fixed(eq)
                rec.update(fixed_equal_spp=eq, fixed_equal_ms=round(ems, 3), rmse_fixed_equal_vs_max=rmse(efb, ref))
            emit(rec)
    art.reset_options()
    ds.close()


if __name__ == "__main__":
    main()
