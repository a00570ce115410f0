#!/usr/bin/env python3
"""What following moved quads buys the temporal accumulation, on an MI355X (profiles/reproject_quads_quality.json).

A scene with boxes (default: the Cornell box) under a still camera, its boxes changing height by the rule of `rayTracer --grow`
(--amount) over --frames frames of --ns samples each.  Every frame gets seeds of its own (seed_base + k nx ny), as
tools/reproject_moving_quality.py explains.  Three images of the last frame -- the single frame, TemporalAccumulator without
following (the updates made on the scene directly) and with follow_quads=True -- against a --ref-ns render of that last state: RMSE
of the linear image over the pixels that show a moved quad and over the whole frame, the same over the moved-quad pixels for which
only the following accumulator found a history, and the share of the moved-quad pixels that found a history in either mode.  The
same at amount 0 is the control: nothing moves and both accumulators give rt_reproject's result.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import accelerated_ray_tracer_amd as art  # noqa: E402
from bench_reproject import box_firsts, grown_boxes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell")
    ap.add_argument("--nx", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=800)
    ap.add_argument("--ns", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--amount", type=float, default=0.2)
    ap.add_argument("--ref-ns", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    art.init(0)
    line = measure(args, args.amount)
    control = measure(args, 0.0)
    line["control_at_rest"] = {k: control[k] for k in ("moved_quad_pixels", "rmse_moved_quad_pixels", "rmse_whole_frame",
                                                       "moved_quad_pixels_with_history", "mean_history_length_on_moved_quads")}
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")


def measure(args, amount):
    nx, ny = args.nx, args.ny
    hs = art.HostScene(args.scene, nx, ny)
    base = hs.quads().copy()
    firsts = box_firsts(base)
    faces = [q for f in firsts for q in range(f, f + 6) if q != f + 5]     # (make_box's last face is the bottom: it stays)
    cam = art.RtCamera.from_buffer_copy(hs.desc.camera)
    images, lengths = {}, {}
    for mode in ("without_following", "with_following"):
        ds = art.DeviceScene(hs)
        acc = art.TemporalAccumulator(ds, hs.frame(nx=nx, ny=ny, ns=args.ns), follow_quads=(mode == "with_following"))
        for k in range(args.frames):
            acc.frame.seed_base = acc.aov_frame.seed_base = 1984 + k * nx * ny
            rec = grown_boxes(base, 1.0 + amount * math.sin(2.0 * math.pi * k / args.frames))
            if mode == "with_following":
                out = acc.push(cam, quads=rec)
            else:
                ds.update_quads(rec)
                out = acc.push(cam)
        images[mode], lengths[mode] = out.copy(), acc.length.copy()
        if mode == "with_following":            # the last state: the single frame, the ids and the reference
            f = hs.frame(nx=nx, ny=ny, ns=args.ns, gamma=1.0, seed_base=1984 + (args.frames - 1) * nx * ny)
            images["single_frame"] = ds.render(f)[0].copy()
            aov = ds.render_aov(f, albedo=False, ids=True)
            reference = ds.render(hs.frame(nx=nx, ny=ny, ns=args.ref_ns, gamma=1.0, seed_base=1984 + args.frames * nx * ny))[0].copy()
        ds.close()
    prim = aov["prim"].astype(np.int64)
    on_moved = (prim >= 0) & ((prim >> 28) == art.RT_PRIM_QUAD) & np.isin(prim & 0x0FFFFFFF, faces) & (aov["alpha"] >= 0.5)

    def rmse(img, mask=None):
        d = (img.astype(np.float64) - reference.astype(np.float64)) ** 2
        return float(np.sqrt(d[mask].mean() if mask is not None else d.mean()))
    gained = on_moved & (lengths["with_following"] > 1) & (lengths["without_following"] == 1)
    line = {"what": "accumulation of a still camera over boxes that change height against a reference of the last state", "scene": args.scene,
            "nx": nx, "ny": ny, "ns": args.ns, "frames": args.frames, "amount": amount, "reference_ns": args.ref_ns,
            "boxes": len(firsts), "moved_quad_pixels": int(on_moved.sum()), "moved_quad_pixel_share": round(float(on_moved.mean()), 4),
            "rmse_moved_quad_pixels": {k: round(rmse(v, on_moved), 5) for k, v in images.items()},
            "pixels_only_following_finds_a_history_for": int(gained.sum()),
            "rmse_on_those_pixels": {k: round(rmse(v, gained), 5) if gained.any() else None for k, v in images.items()},
            "rmse_whole_frame": {k: round(rmse(v), 5) for k, v in images.items()},
            "moved_quad_pixels_with_history": {k: round(float((v[on_moved] > 1).mean()), 4) for k, v in lengths.items()},
            "mean_history_length_on_moved_quads": {k: round(float(v[on_moved].mean()), 3) for k, v in lengths.items()},
            "mean_history_length_on_those_pixels": round(float(lengths["with_following"][gained].mean()), 3) if gained.any() else None}
    hs.close()
    return line


if __name__ == "__main__":
    main()
