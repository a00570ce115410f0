#!/usr/bin/env python3
"""Quality record behind DESIGN.md 4.13: the experiment of 4.11 / 4.12 -- the oracle at 4 spp, 96 x 64, filtered with the
expectation of both filters (tests/denoise_expect.py, tests/variance_expect.py) at the binding's defaults, against the oracle
at 256 spp and another seed -- with the guides taken THROUGH mirrors and glass (tests/aov_through_expect.py) in place of the
first-hit feature buffers, at max_bounces 2 and 8 and fuzz_limit 0, 0.3 and 1.  Prints RMSE(filtered) / RMSE(noisy) per frame.

Two stages, because the expectation's albedo of textured terminals and of the gradient miss term is DeviceScene.radiance of
the emissive twin (normal and depth are the oracle's alone):
  --albedo-out FILE   (needs a GPU, seconds) the through-albedo of every frame and setting, written to an .npz;
  --albedo-in FILE    (no GPU, minutes) the filters in NumPy on those, the table on stdout and, with --json FILE, the figures;
                      --golden FILE also writes the albedo the host test reads (tests/test_aov_through_host.py): the frames of
                      GOLDEN at the binding's default setting.
With neither, both stages run in this process (a GPU is needed then)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import accelerated_ray_tracer_amd as art   # noqa: E402
import oracle as orc                       # noqa: E402
import aov_expect as ax                    # noqa: E402
import aov_through_expect as tx            # noqa: E402
import denoise_expect as dx                # noqa: E402
import variance_expect as vx               # noqa: E402

FRAMES = ["spheres_plain/1", "spheres_tex/3", "general_plain/1", "general_tex/4", "bouncing", "final"]
NX, NY, NS, B = 96, 64, 4, 4
SETTINGS = [(mb, fz) for mb in (2, 8) for fz in (0.0, 0.3, 1.0)]
GOLDEN = ["spheres_plain/1", "general_plain/1"]   # the frames the host test asserts (73 KB each before compression)


def tag(key, mb, fz):
    return f"{key}|{mb}|{fz:g}"


def through_albedo():
    """{tag: albedo} for every frame and setting, with the twins on the device."""
    import torch   # noqa: F401  (before the render library initialises the device: both then share one HIP runtime)
    art.init(0)
    out = {}
    for key in FRAMES:
        case = ax.Case(art, orc, key)
        twin = art.DeviceScene(case.twin)
        try:
            for mb, fz in SETTINGS:
                e = tx.expected(case, NX, NY, NS, mb, fz, twin)
                assert not np.isnan(e["albedo"]).any()
                out[tag(key, mb, fz)] = e["albedo"]
        finally:
            twin.close()
        print(key, "albedo done", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--albedo-out")
    ap.add_argument("--albedo-in")
    ap.add_argument("--json")
    ap.add_argument("--golden")
    a = ap.parse_args()
    orc.lib()
    if a.albedo_out:
        np.savez_compressed(a.albedo_out, **through_albedo())
        return
    albedo = dict(np.load(a.albedo_in)) if a.albedo_in else through_albedo()
    shared = {k: art.DENOISE_DEFAULTS[k] for k in ("iterations", "normal_sharpness", "sigma_depth")}
    rows, share = {}, {}
    for key in FRAMES:
        f = vx.oracle_frame(art, orc, key, ns=NS, batches=B, nx=NX, ny=NY)
        truth, _ = f["oracle"].render(256, gamma=1.0, seed_base=77_000_000_019)

        def rmse(x):
            return float(np.sqrt(np.mean((x.astype(np.float64) - truth) ** 2)))
        noisy = rmse(f["color"])

        def both(name, alb, nrm, dep):
            rows.setdefault(f"colour factor, {name}", {})[key] = rmse(dx.denoise(f["color"], alb, nrm, dep, **art.DENOISE_DEFAULTS)) / noisy
            out, _ = vx.denoise_variance(f["color"], f["variance"], alb, nrm, dep, **shared, **art.DENOISE_VARIANCE_DEFAULTS)
            rows.setdefault(f"variance-guided, {name}", {})[key] = rmse(out) / noisy
        both("first hit (shipped)", f["albedo"], f["normal"], f["depth"])
        for mb, fz in SETTINGS:
            e = tx.expected(f["case"], NX, NY, NS, mb, fz, None)          # normal and depth: the oracle's alone
            alb = albedo[tag(key, mb, fz)]
            known = ~e["device_needed"].any(axis=2)
            assert np.array_equal(alb[known].view(np.uint32), e["albedo"][known].view(np.uint32)), (key, mb, fz)
            both(f"through {mb}, {fz:g}", alb, e["normal"], e["depth"])
            share[tag(key, mb, fz)] = float((e["chain"]["k"] >= 1).mean())
        print(key, "done", file=sys.stderr, flush=True)
    print("| filter, guides (max_bounces, fuzz_limit) | " + " | ".join(FRAMES) + " |")
    print("|---|" + "---|" * len(FRAMES))
    for name, r in rows.items():
        print(f"| {name} | " + " | ".join(f"{r[k]:.3f}" for k in FRAMES) + " |")
    print("| share of samples followed, 8 bounces, fuzz_limit 0 / 0.3 / 1 | "
          + " | ".join(" / ".join(f"{share[tag(k, 8, fz)]:.3f}" for fz in (0.0, 0.3, 1.0)) for k in FRAMES) + " |")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"nx": NX, "ny": NY, "ns": NS, "batches": B, "ratio": rows, "share_followed": share}, fh, indent=1)
    if a.golden:
        d = art.AOV_THROUGH_DEFAULTS
        np.savez_compressed(a.golden, **{k: albedo[tag(k, d["max_bounces"], d["fuzz_limit"])] for k in GOLDEN})


if __name__ == "__main__":
    main()
