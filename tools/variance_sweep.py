#!/usr/bin/env python3
"""CPU sweep behind DENOISE_VARIANCE_DEFAULTS: the variance-guided filter's expectation
(tests/variance_expect.py) on the frames of DESIGN.md 4.11's table -- the oracle at 4 spp, 96 x 64, oracle-side feature
buffers, variance by batch means at B = 4 -- against the oracle at 256 spp and another seed.  Prints RMSE(filtered) /
RMSE(noisy) per frame for the shipped colour-factor settings and for a grid of (sigma_variance, variance_floor).  No GPU."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import accelerated_ray_tracer_amd as art   # noqa: E402
import oracle as orc                       # noqa: E402
import denoise_expect as dx                # noqa: E402
import variance_expect as vx               # noqa: E402

FRAMES = ["spheres_plain/1", "spheres_tex/3", "general_plain/1", "general_tex/4", "bouncing", "final"]
NX, NY, NS, B = 96, 64, 4, 4
GRID = [(s, fl) for s in (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0) for fl in (1e-6, 1e-4, 1e-2)]


def main():
    orc.lib()
    rows = {}
    for key in FRAMES:
        f = vx.oracle_frame(art, orc, key, ns=NS, batches=B, nx=NX, ny=NY)
        truth, _ = f["oracle"].render(256, gamma=1.0, seed_base=77_000_000_019)

        def rmse(a):
            return float(np.sqrt(np.mean((a.astype(np.float64) - truth) ** 2)))
        noisy = rmse(f["color"])
        guides = (f["albedo"], f["normal"], f["depth"])
        rows.setdefault("colour factor (shipped)", {})[key] = rmse(dx.denoise(f["color"], *guides, **art.DENOISE_DEFAULTS)) / noisy
        shared = {k: art.DENOISE_DEFAULTS[k] for k in ("iterations", "normal_sharpness", "sigma_depth")}
        for s, fl in GRID:
            out, _ = vx.denoise_variance(f["color"], f["variance"], *guides, sigma_variance=s, variance_floor=fl, **shared)
            rows.setdefault(f"variance {s:g}, {fl:g}", {})[key] = rmse(out) / noisy
        print(key, "done", file=sys.stderr, flush=True)
    print("| settings | " + " | ".join(FRAMES) + " |")
    print("|---|" + "---|" * len(FRAMES))
    for name, r in rows.items():
        print(f"| {name} | " + " | ".join(f"{r[k]:.3f}" for k in FRAMES) + " |")
    print(json.dumps(rows), file=sys.stderr)


if __name__ == "__main__":
    main()
