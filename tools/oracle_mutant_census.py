#!/usr/bin/env python3
"""Which frames of the render corpus notice which planted error of the oracle (tests/oracle_mutants.py)?  CPU only.

The corpus is the (scene, size, spp) list of the GPU render tests, read from the test modules themselves: the parametrize lists
of tests/test_gpu_parity.py (test_scene_matches_oracle, test_walk_array_is_invisible, the schedule and hand-off tests, the
progressive windows at their 24 samples), the generated scenes of tests/test_desc_parity.py (test_desc_oracle.LIVE), the scenes
of tests/test_kernel_matrix.py at both its frames and its big scenes, tests/test_carried_constants.py's scenes and its
re-cameraed and re-skied frames; with --edges the edge scenes of tests/edge_scenes.py instead.
Per mutant: the frames whose pixels or ray count differ from the unmutated oracle's (the search stops at --enough kills).
One JSON line per mutant on stdout.  profiles/edge_scenes_tests_mutations.md holds a run.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import accelerated_ray_tracer_amd as art  # noqa: E402
import oracle  # noqa: E402
import oracle_mutants as om  # noqa: E402
import scene_gen as sg  # noqa: E402
import test_desc_oracle as tdo  # noqa: E402
import test_kernel_matrix_host as km  # noqa: E402

def _cases(fn):
    """The argument list of a test's first parametrize mark."""
    return list(fn.pytestmark[-1].args[1])


def corpus(edges):
    """[(label, make(orc) -> OracleScene, ns, seed_base)], without repeats."""
    if edges:
        import edge_scenes as es
        return [(e.name, (lambda o, e=e: o.OracleScene.from_host(e.scene)), es.NS, e.seed_base) for e in es.EDGES]
    import reproject_expect as rx
    import test_carried_constants as tcc
    import test_gpu_parity as tgp
    out, seen = [], set()

    def named(name, nx, ny, ns, why):
        if (name, nx, ny, ns) in seen:
            return
        seen.add((name, nx, ny, ns))
        img, iw, ih = art.default_texture(name)
        out.append((f"{why} {name} {nx}x{ny} {ns}spp", (lambda o, a=(name, nx, ny, img, iw, ih): o.OracleScene(*a)), ns, 1984))

    def described(label, hs, nx, ny, ns):
        out.append((f"{label} {nx}x{ny} {ns}spp", (lambda o, hs=hs, nx=nx, ny=ny: o.OracleScene.from_host(hs, nx, ny)), ns, 1984))

    for fn in (tgp.test_scene_matches_oracle, tgp.test_walk_array_is_invisible, tgp.test_split_frame_schedule_matches_oracle,
               tgp.test_tail_handoff_matches_oracle):
        for name, nx, ny, ns in _cases(fn):
            named(name, nx, ny, ns, "parity")
    for name, nx, ny in _cases(tgp.test_progressive_windows_equal_one_shot):
        named(name, nx, ny, 24, "parity")
    for recipe, seed, nx, ny in tdo.LIVE:
        described(f"desc {recipe}/{seed}", sg.generate(recipe, seed, nx, ny), nx, ny, tdo.NS)
    for key in km.SCENES:
        for nx, ny, ns in ((km.NX, km.NY, km.NS), (km.SNX, km.SNY, km.SNS)):
            hs = km.load(art, key, nx, ny)
            out.append((f"matrix {key} {nx}x{ny} {ns}spp", (lambda o, a=(key, hs, nx, ny): km.oracle_of(o, art, *a)), ns, 1984))
    for family in km.FAMILIES:
        for ns in (2, 4):
            described(f"matrix big/{family}", km.big_scene(family), km.SNX, km.SNY, ns)
    for name in tcc.WALK_SCENES:
        if "/" not in name:
            named(name, tcc.NX, tcc.NY, tcc.NS, "carried")
    for case, c in tcc.FRAMES.items():                           # the re-cameraed and re-skied frames of test_records_read_in_stage_e
        nx, ny = c.get("size", (tcc.NX, tcc.NY))
        hs = art.HostScene("bouncing", nx, ny)
        if "aperture" in c:
            hs = rx.WithCamera(art, hs, tcc._orbited(art, nx, ny, c["aperture"]))
        if "sky" in c:
            hs = tcc._Sky(art, hs, *c["sky"])
        described(f"carried bouncing/{case}", hs, nx, ny, tcc.NS)
    hs = art.HostScene("bouncing", tcc.NX, tcc.NY)
    described("carried bouncing/orbited", rx.WithCamera(art, hs, tcc._orbited(art, tcc.NX, tcc.NY, 0.1)), tcc.NX, tcc.NY, tcc.NS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", action="store_true")
    ap.add_argument("--enough", type=int, default=2)
    ap.add_argument("--mutants", nargs="*", default=om.NAMES)
    a = ap.parse_args()
    frames = corpus(a.edges)
    oracle.lib()
    ref = [make(oracle).render(ns, seed_base=seed) for _, make, ns, seed in frames]
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(0, len(a.mutants), om.MAX_BUILDS):
            for name, handle in om.build(a.mutants[k:k + om.MAX_BUILDS], tmp).items():
                killed = []
                with om.using(handle) as mo:
                    for (label, make, ns, seed), (fb, cnt) in zip(frames, ref):
                        got, c = make(mo).render(ns, seed_base=seed)
                        if c != cnt or not np.array_equal(got.view(np.uint32), fb.view(np.uint32)):
                            killed.append(label)
                            if len(killed) >= a.enough:
                                break
                print(json.dumps({"mutant": name, "frames": len(frames), "killed_by": killed, "stopped_early": len(killed) >= a.enough}), flush=True)


if __name__ == "__main__":
    main()
