"""The conditions on tests/edge_scenes.py, from the oracle alone: no device.

1. Every planted error of tests/oracle_mutants.py changes the pixels or the ray count of at least one edge scene, unless it
   stands in UNREACHABLE with an argument that no ray of a render reaches the branch.  A scene that kills a mutant is a frame in
   which the mutated rule decides; rendered on the kernels bit for bit (tests/test_edge_scenes.py) it pins the rule there.
2. The designed ties are exact: the oracle's trace() of the primary ray gives the expected winner at the expected t, and each
   tied candidate alone is met at the bit-equal t.
3. The description oracle takes these scenes as it takes the generated ones (counters the contents imply, a tree that is
   binary, finite frames).

Each mutant renders only the scenes built for its rule and, if none of them kills it, every scene: the module's report
(-s) shows which scene killed which mutant.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_scenes as es
import oracle_mutants as om

# Mutants no ray of a render can tell from the oracle, each with the reason.  Not a place for scenes that were hard to build.
UNREACHABLE = {
    "medium_no_zero_clamp": "the line before it raises rec1.t to tmin, and every caller of the world's hit passes tmin = 0.001 "
                            "(the integrator, rt_trace_rays' default and the feature passes): rec1.t >= 0.001 > 0 when `rec1.t < 0` is asked",
    "image_no_clamp01": "every producer of (u, v) stays in [0, 1]: sphere_uv divides phi in [0, 2 pi] and theta in [0, pi] by their "
                        "upper bounds (float division of x by y >= x gives at most 1), a quad stores alpha, beta only after the test "
                        "0 <= . <= 1, a medium stores 0, and uv_offset wraps u into [0, 1) and clamps v to [0, 1] before the lookup",
    "uvoff_no_clamp": "the only texture that reads v is the image (a checker hands u, v on, a nested uv_offset clamps again), and its own "
                      "first act is v = clamp01(v): the same value for every v that is not a NaN, and v is a sum of two finite numbers",
    "quad_flip_lax": "vdot(n, r.d) is the same expression as denom, and |denom| < 1e-8f has already returned: at the flip denom != 0",
}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def reference(orc):
    """Per edge scene: the unmutated oracle's frame and counters, computed once."""
    out = {}
    for e in es.EDGES:
        fb, cnt = orc.OracleScene.from_host(e.scene).render(es.NS, seed_base=e.seed_base)
        out[e.name] = (fb, cnt)
    return out


@pytest.fixture(scope="module")
def kills():
    """oracle_mutants.kill_table(), computed in a process of its own: the mutant libraries never share a process with the suite
    (which on a GPU machine holds the device)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.dirname(os.path.abspath(__file__))] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, om.__file__], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    result = json.loads(r.stdout.strip().splitlines()[-1])
    for name in om.NAMES:
        print(f"{name:28s} {'UNREACHABLE' if name in UNREACHABLE else ''} killed by {result[name]}")
    return result


def test_mutant_texts_apply_exactly_once():
    for name in om.NAMES:
        assert om.mutated_text(name) != open(om.SOURCE).read(), name
    with pytest.raises(LookupError):
        om.mutated_text("sphere_disc_lax", "no such text")
    with pytest.raises(LookupError):
        om.mutated_text("sphere_disc_lax", "if (disc <= 0.0f) return false;" * 2)


@pytest.mark.parametrize("name", om.NAMES)
def test_every_mutant_is_killed(kills, name):
    if name in UNREACHABLE:
        assert not kills[name], f"{name} is listed as unreachable and {kills[name]} reaches it: take it out of the table"
    else:
        assert kills[name], f"no edge scene notices {name}"


def test_scenes_kill_what_they_were_built_for(kills):
    """A scene's `rules` are claims: each named mutant does change that scene."""
    for e in es.EDGES:
        for rule in e.rules:
            assert e.name in kills[rule], (e.name, rule, kills[rule])


@pytest.mark.parametrize("name", [e.name for e in es.EDGES + es.PADDED])
def test_designed_ties_are_exact(orc, name):
    e = es.BY_NAME[name]
    t, p, n, uv, mat = orc.OracleScene.from_host(e.scene).trace(e.o[None], e.d[None])
    if e.winner_mat is not None:
        assert int(mat[0]) == e.winner_mat, (name, int(mat[0]), e.winner_mat, float(t[0]))
    if e.t is not None and e.winner_mat is not None:
        assert _bits(t)[0] == _bits(e.t), (name, float(t[0]))
    for s in e.solos:
        ts = orc.OracleScene.from_host(s).trace(e.o[None], e.d[None])[0]
        assert _bits(ts)[0] == _bits(t)[0], (name, float(ts[0]), float(t[0]))
    if len(e.solos) > 1:
        assert e.t is not None


@pytest.mark.parametrize("name", [e.name for e in es.EDGES])
def test_oracle_takes_the_scene(orc, reference, name):
    e = es.BY_NAME[name]
    g = e.scene
    fb, cnt = reference[name]
    assert np.isfinite(fb).all()
    assert cnt["samples"] == es.NX * es.NY * es.NS and cnt["rays"] >= cnt["samples"]
    d = g.desc
    implied = {k for k, n in (("sphere_tests", d.n_spheres), ("quad_tests", d.n_quads), ("box6_calls", d.n_boxes),
                              ("inst_calls", d.n_instances), ("medium_calls", d.n_media)) if n}
    assert implied == set(g.contents)
    for k in implied - {"sphere_tests"}:                       # (the far fillers' boxes are missed: their spheres may never be tested)
        assert cnt[k] > 0, (k, cnt)
    n = g.nodes()
    assert len(n) == 2 * g.n_leaves - 1 and n["skip"][0] == len(n)
    # every sample of every pixel starts with the same ray: the oracle's own camera says so
    o = orc.OracleScene.from_host(g)
    cam = o.camera()
    assert np.array_equal(cam[0:3], e.o) and np.array_equal(cam[3:6] - cam[0:3], e.d), cam
    assert not cam[6:12].any(), cam


def test_the_list_holds_what_it_promises():
    names = set(es.BY_NAME)
    for group in ("spheres/", "quads/", "mixed/", "box/", "instance/", "quad-edge/", "grazing/", "medium/", "texture/", "seeded/", "padded/"):
        assert any(n.startswith(group) for n in names), group
    for e in es.EDGES:
        if "63-64" in e.name:                                   # the last two tied parts are the leaves of ordinal 63 and 64
            prim = e.scene.nodes()["prim"]
            leaves = prim[prim >= 0]
            spheres, r = e.scene.spheres(), leaves[63:65] & 0x0FFFFFFF
            filler = [(p >> 28) == 0 and float(spheres["c0"][i][2]) == -50.0 for p, i in zip(leaves[63:65], r)]
            assert e.scene.n_leaves >= 65 and not any(filler), (e.name, leaves[63:65])
            assert {63, 64} <= set(e.scene.part_mats), (e.name, sorted(e.scene.part_mats))
    assert es.PADDED[0].scene.n_leaves > es.BIG_LEAVES
    assert all(x != 0 for x in es.D)                           # three non-zero components: the tier wave keeps its reduction
