#!/usr/bin/env python3
"""What following moved spheres buys the temporal accumulation, on an MI355X (profiles/reproject_moving_quality.json).

The headline scene under a still camera, its small spheres (radius in (0, 0.5)) bouncing by the rule of `rayTracer --bounce`
(HEIGHT = --height) over --frames frames of --ns samples each.  Every frame gets seeds of its own (seed_base + k nx ny: no
pixel of one frame shares its stream with a pixel of another): under a still camera equal seeds would give static pixels equal
samples, and an average of equal frames converges to nothing.  Three
images of the last frame -- the single frame, TemporalAccumulator without following (the updates made on the scene directly)
and with follow_spheres=True -- against a --ref-ns render of that last state: RMSE of the linear image over the pixels that
show a moved sphere and over the whole frame, the same over the moved-sphere pixels for which only the following accumulator found a history, and
the share of the moved-sphere pixels that found a history in either mode.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import accelerated_ray_tracer_amd as art  # noqa: E402


def records_of_frame(base, k, frames, height):
    rec = base.copy()
    for i in np.flatnonzero((base["radius"] > 0) & (base["radius"] < 0.5)):
        rec["c0"][i, 1] = np.float32(float(base["c0"][i, 1]) + height * abs(math.sin(math.pi * (k / frames + 0.61803398875 * int(i)))))
    return rec


def main():
    """The measurement at --height, and the same at height 0 as a control: there no sphere moves, both accumulators are
    rt_reproject's and every sphere pixel keeps its whole history, so what separates the two records is the motion alone."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=800)
    ap.add_argument("--ns", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=float, default=0.4)
    ap.add_argument("--ref-ns", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    art.init(0)
    line = measure(args, args.height)
    control = measure(args, 0.0)
    line["control_height_0"] = {k: control[k] for k in ("moved_sphere_pixels", "rmse_moved_sphere_pixels", "rmse_whole_frame",
                                                         "moved_sphere_pixels_with_history", "mean_history_length_on_moved_spheres")}
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")


def measure(args, height):
    nx, ny = args.nx, args.ny
    hs = art.HostScene("random_scene", nx, ny)
    base = hs.spheres()
    small = np.flatnonzero((base["radius"] > 0) & (base["radius"] < 0.5))
    cam = hs.desc.camera
    images, lengths = {}, {}
    for mode in ("without_following", "with_following"):
        ds = art.DeviceScene(hs)
        acc = art.TemporalAccumulator(ds, hs.frame(nx=nx, ny=ny, ns=args.ns), follow_spheres=(mode == "with_following"))
        for k in range(args.frames):
            acc.frame.seed_base = acc.aov_frame.seed_base = 1984 + k * nx * ny
            rec = records_of_frame(base, k, args.frames, height)
            if mode == "with_following":
                out = acc.push(cam, spheres=rec)
            else:
                ds.update_spheres(rec)
                out = acc.push(cam)
        images[mode], lengths[mode] = out.copy(), acc.length.copy()
        if mode == "with_following":            # the last state: the single frame, the ids and the reference
            f = hs.frame(nx=nx, ny=ny, ns=args.ns, gamma=1.0, seed_base=1984 + (args.frames - 1) * nx * ny)
            images["single_frame"] = ds.render(f)[0].copy()
            aov = ds.render_aov(f, albedo=False, ids=True)
            reference = ds.render(hs.frame(nx=nx, ny=ny, ns=args.ref_ns, gamma=1.0, seed_base=1984 + args.frames * nx * ny))[0].copy()
        ds.close()
    prim = aov["prim"]
    on_moved = (prim >= 0) & ((prim >> 28) == art.RT_PRIM_SPHERE) & np.isin(prim & 0x0FFFFFFF, small) & (aov["alpha"] >= 0.5)

    def rmse(img, mask=None):
        d = (img.astype(np.float64) - reference.astype(np.float64)) ** 2
        return float(np.sqrt(d[mask].mean() if mask is not None else d.mean()))
    gained = on_moved & (lengths["with_following"] > 1) & (lengths["without_following"] == 1)
    line = {"what": "accumulation of a still camera over bouncing spheres against a reference of the last state", "scene": "random_scene",
            "nx": nx, "ny": ny, "ns": args.ns, "frames": args.frames, "height": height, "reference_ns": args.ref_ns,
            "moved_spheres": int(len(small)), "moved_sphere_pixels": int(on_moved.sum()), "moved_sphere_pixel_share": round(float(on_moved.mean()), 4),
            "rmse_moved_sphere_pixels": {k: round(rmse(v, on_moved), 5) for k, v in images.items()},
            "pixels_only_following_finds_a_history_for": int(gained.sum()),
            "rmse_on_those_pixels": {k: round(rmse(v, gained), 5) if gained.any() else None for k, v in images.items()},
            "rmse_whole_frame": {k: round(rmse(v), 5) for k, v in images.items()},
            "moved_sphere_pixels_with_history": {k: round(float((v[on_moved] > 1).mean()), 4) for k, v in lengths.items()},
            "mean_history_length_on_moved_spheres": {k: round(float(v[on_moved].mean()), 3) for k, v in lengths.items()},
            "mean_history_length_on_those_pixels": round(float(lengths["with_following"][gained].mean()), 3) if gained.any() else None}
    hs.close()
    return line


if __name__ == "__main__":
    main()
