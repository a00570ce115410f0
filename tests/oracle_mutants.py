"""Planted errors of the CPU oracle, as data: what tests/test_edge_scenes_host.py asks the edge scenes to notice.

Each entry of MUTANTS is one edit of oracle/rt_oracle.cpp -- a comparison made strict or lax, a guard removed, an order reversed --
on a rule that decides a pixel only where two t are equal or a value sits exactly on a boundary.  A kernel carrying the same
error agrees with the oracle on every frame in which the rule never decides; a scene kills a mutant when the mutated oracle's
frame or ray count differs from the unmutated one's, and only then does the scene pin the rule on the kernels.

`find` must occur in the oracle's text exactly once, otherwise mutated_text() raises: an edit of the oracle cannot silently
disarm a mutant.  build() writes the mutated texts into a temporary directory and compiles them through oracle/Makefile's pattern
rule (the library's own compiler and flags), at most 16 at a time; each library is loaded through a ctypes handle of its own
(oracle.load).  Nothing mutated is kept.  CPU-only test infrastructure: kill_table() is run as a program of its own (`python
tests/oracle_mutants.py`, as tests/test_edge_scenes_host.py does), so that no mutant is loaded into a process that may hold the GPU.
"""
from __future__ import annotations

import contextlib
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import oracle

SOURCE = os.path.join(os.path.dirname(os.path.realpath(oracle.__file__)), "rt_oracle.cpp")
MAX_BUILDS = 16

_SPHERE_ROOTS = """    if (!(t > tmin && t < tmax)) {
        t = (-b + sq) / a;
        if (!(t > tmin && t < tmax)) return false;
    }"""

# (name, find, replace, the rule it breaks)
MUTANTS = [
    # ---- the limits a hit is accepted against
    ("quad_tmax_strict", "if (t < tmin || t > tmax) return false;", "if (t < tmin || t >= tmax) return false;",
     "quad::hit accepts t <= limit: of two quads at equal t the later one wins"),
    ("sphere_tmax_lax", _SPHERE_ROOTS, _SPHERE_ROOTS.replace("t < tmax", "t <= tmax"),
     "sphere::hit accepts t < limit: of two spheres at equal t the earlier one wins"),
    ("bvh_left_lax", "if (hl && (!hr || lrec.t < rrec.t)) rec = lrec;", "if (hl && (!hr || lrec.t <= rrec.t)) rec = lrec;",
     "bvh_hit keeps the left record only if it is strictly closer"),
    ("quad_tmin_lax", "if (t < tmin || t > tmax) return false;", "if (t <= tmin || t > tmax) return false;",
     "quad::hit accepts t == tmin"),
    ("sphere_tmin_lax", _SPHERE_ROOTS, _SPHERE_ROOTS.replace("t > tmin", "t >= tmin"),
     "sphere::hit rejects t == tmin"),
    ("sphere_disc_lax", "if (disc <= 0.0f) return false;", "if (disc < 0.0f) return false;",
     "a tangent ray (disc == 0) misses the sphere"),
    ("box6_reversed", "for (int i = 0; i < 6; ++i) {\n        Hit tmp;", "for (int i = 5; i >= 0; --i) {\n        Hit tmp;",
     "a box scans its faces 0..5: on an edge or a corner the last face at the smallest t wins"),
    # ---- a quad's edges
    ("quad_edge_hi_out", "if (alpha < 0.f || alpha > 1.f || beta < 0.f || beta > 1.f) return false;",
     "if (alpha < 0.f || alpha >= 1.f || beta < 0.f || beta >= 1.f) return false;", "alpha == 1 and beta == 1 are inside the quad"),
    ("quad_edge_lo_out", "if (alpha < 0.f || alpha > 1.f || beta < 0.f || beta > 1.f) return false;",
     "if (alpha <= 0.f || alpha > 1.f || beta <= 0.f || beta > 1.f) return false;", "alpha == 0 and beta == 0 are inside the quad"),
    ("quad_denom_lax", "if (fabsf(denom) < 1e-8f) return false;", "if (fabsf(denom) <= 1e-8f) return false;",
     "|denom| == 1e-8f is not parallel"),
    ("quad_denom_unguarded", "if (fabsf(denom) < 1e-8f) return false;", "",
     "a ray parallel to the quad's plane misses it"),
    # ---- a medium's interval
    ("medium_empty_strict", "if (rec1.t >= rec2.t) return false;", "if (rec1.t > rec2.t) return false;",
     "an interval clipped to nothing (entry == limit) holds no medium"),
    ("medium_exit_lax", "if (hit_distance > distance_inside) return false;", "if (hit_distance >= distance_inside) return false;",
     "a scatter exactly at the interval's end is inside"),
    ("medium_no_floor", "float U = fmaxf(1e-6f, rng_uniform(fake));", "float U = rng_uniform(fake);",
     "the medium's uniform is at least 1e-6"),
    ("medium_no_zero_clamp", "if (rec1.t < 0) rec1.t = 0;", "", "a medium's entry is never negative"),
    ("medium_no_tmax_clip", "if (rec2.t > tmax) rec2.t = tmax;", "", "a medium's exit is clipped to the limit it is handed"),
    ("medium_no_tmin_clip", "if (rec1.t < tmin) rec1.t = tmin;", "", "a medium's entry is clipped to tmin"),
    ("medium_exit_from_entry", "if (!obj_hit(m->child, r, rec1.t + 1e-4f, FLT_MAX, rec2)) return false;",
     "if (!obj_hit(m->child, r, rec1.t, FLT_MAX, rec2)) return false;", "the exit is searched from entry + 1e-4"),
    # ---- the limit through the wrappers
    ("translate_drops_limit", "if (!obj_hit(t->child, moved, tmin, tmax, rec)) return false;",
     "if (!obj_hit(t->child, moved, tmin, FLT_MAX, rec)) return false;", "translate hands its limit to its child"),
    ("roty_drops_limit", "if (!obj_hit(ro->child, rr, tmin, tmax, rec)) return false;",
     "if (!obj_hit(ro->child, rr, tmin, FLT_MAX, rec)) return false;", "rotate_y hands its limit to its child"),
    # ---- signs at exactly zero
    ("metal_grazing_lax", "return vdot(out.d, rec.n) > 0.0f;", "return vdot(out.d, rec.n) >= 0.0f;",
     "a metal scatter along the surface is absorbed"),
    ("dielectric_grazing_lax", "if (vdot(in.d, rec.n) > 0.0f) {\n            outward = vneg(rec.n);", "if (vdot(in.d, rec.n) >= 0.0f) {\n            outward = vneg(rec.n);",
     "a ray along a glass surface counts as entering"),
    ("quad_flip_lax", "if (vdot(n, r.d) > 0.f) n = vneg(n);", "if (vdot(n, r.d) >= 0.f) n = vneg(n);", "a quad's normal flips only against a ray strictly along it"),
    ("roty_flip_lax", "if (vdot(rec.n, r.d) > 0.f) rec.n = vneg(rec.n);", "if (vdot(rec.n, r.d) >= 0.f) rec.n = vneg(rec.n);",
     "rotate_y's normal flips only against a ray strictly along it"),
    ("dielectric_prob_lax", "if (rng_uniform(g) < reflect_prob) out.d = refl; else out.d = refr;",
     "if (rng_uniform(g) <= reflect_prob) out.d = refl; else out.d = refr;", "glass reflects when uniform < reflect_prob"),
    # ---- textures
    ("image_column_clamp", "if (i > t->w - 1) i = t->w - 1;", "if (i > t->w) i = t->w - 1;", "u == 1 reads the last column"),
    ("image_row_clamp", "if (j > t->h - 1) j = t->h - 1;", "if (j > t->h) j = t->h - 1;", "v == 0 reads the last row"),
    ("image_no_clamp01", "u = clamp01(u); v = clamp01(v);", "", "u, v are clamped to [0, 1] before the lookup"),
    ("light_ignores_texture", "return m->tex ? tex_value(m->tex, u, v, p) : m->albedo;", "return m->albedo;", "a textured light emits its texture"),
    ("checker_parity", "bool is_even = ((xi + yi + zi) & 1) == 0;", "bool is_even = ((xi + yi + zi) & 1) != 0;", "an even cell sum takes the first texture"),
    ("uvoff_no_wrap", "float uu = u + t->du; uu -= floorf(uu);", "float uu = u + t->du;", "uv_offset wraps u"),
    ("uvoff_no_clamp", "vv = fminf(fmaxf(vv, 0.f), 1.f);", "", "uv_offset clamps v"),
    # ---- the slab test
    ("slab_tie_lax", "if (tmax <= tmin) return false;", "if (tmax < tmin) return false;", "a box met in a single point is missed"),
]
NAMES = [m[0] for m in MUTANTS]
assert len(set(NAMES)) == len(NAMES)


def mutated_text(name: str, text: str | None = None) -> str:
    if text is None:
        with open(SOURCE) as f:
            text = f.read()
    _, find, replace, _ = MUTANTS[NAMES.index(name)]
    if text.count(find) != 1:
        raise LookupError(f"mutant {name}: its text occurs {text.count(find)} times in rt_oracle.cpp, not once")
    return text.replace(find, replace)


def _compile(cpp: str) -> str:
    so = cpp[:-4] + ".so"
    r = subprocess.run(["make", "-C", os.path.dirname(SOURCE), so], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{cpp} does not build:\n{r.stdout}{r.stderr}")
    return so


def build(names, directory: str) -> dict:
    """name -> a handle of its own on the mutant's library, built under `directory` (a temporary one: the caller removes it)."""
    with open(SOURCE) as f:
        text = f.read()
    sources = []
    for name in names:
        path = os.path.join(directory, f"mutant_{name}.cpp")
        with open(path, "w") as f:
            f.write(mutated_text(name, text))
        sources.append(path)
    with ThreadPoolExecutor(MAX_BUILDS) as pool:
        libs = list(pool.map(_compile, sources))
    return {name: oracle.load(so) for name, so in zip(names, libs)}


@contextlib.contextmanager
def using(handle):
    """The oracle binding on another library for the length of the block.  A scene is used under the handle that created it."""
    old = oracle._lib
    oracle._lib = handle
    try:
        yield oracle
    finally:
        oracle._lib = old


def kill_table(names=None) -> dict:
    """mutant -> the edge scenes (tests/edge_scenes.py) whose frame or counters it changes: searched first among the scenes built
    for it, and among all the others only if none of those does."""
    import tempfile

    import numpy as np

    import edge_scenes as es
    names = list(NAMES if names is None else names)
    oracle.lib()
    reference = {e.name: oracle.OracleScene.from_host(e.scene).render(es.NS, seed_base=e.seed_base) for e in es.EDGES}
    result = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(0, len(names), MAX_BUILDS):
            for name, handle in build(names[k:k + MAX_BUILDS], tmp).items():
                killed = []
                with using(handle) as mo:
                    for group in ([e for e in es.EDGES if name in e.rules], [e for e in es.EDGES if name not in e.rules]):
                        for e in group:
                            fb, cnt = mo.OracleScene.from_host(e.scene).render(es.NS, seed_base=e.seed_base)
                            ref_fb, ref_cnt = reference[e.name]
                            if cnt != ref_cnt or not np.array_equal(fb.view(np.uint32), ref_fb.view(np.uint32)):
                                killed.append(e.name)
                        if killed:
                            break
                result[name] = killed
    return result


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    print(json.dumps(kill_table(sys.argv[1:] or None)))
