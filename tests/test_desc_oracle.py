"""The description oracle (orc_scene_from_desc, OracleScene.from_desc) anchored on the CPU, and the generated scenes' liveness.

Parity chain: the reference's images pin the named oracle (tests/test_reference_images.py); the named oracle pins the
description oracle here -- fed the description the host library flattens for a named scene, it must give the named oracle's
frame, counters, tree and ray answers bit for bit; the description oracle then checks the kernels on descriptions nobody
wrote by hand (tests/test_desc_parity.py, tests/scene_gen.py).  If the two oracles disagree the new code is wrong: the named
path is not touched.

No GPU is needed for anything in this module.
"""
import numpy as np
import pytest

import scene_gen as sg
import trace_families as tf

# every name of test_gpu_parity.test_scene_matches_oracle
NAMED = ["two_spheres", "bouncing", "book1", "cornell", "cornell_smoke", "final", "degenerate", "checker", "earth", "perlin", "quads",
         "simple_light", "original", "instanced", "fog", "crowd_4096", "crowd_4097", "crowd_2400", "crowd_big"]

# The (recipe, seed) list of the GPU tests (tests/test_desc_parity.py).  Fixed: a seed stays once it is here, and one that ever
# exposes a mismatch is added.  `limits` takes every leaf count, spheres only (0..8) and with one quad (9..17).
# general_*: five seeds, so that the media cycle through 0, 1 and 2 of them and every boundary kind (scene_gen.GENERAL_MEDIA).
SEEDS = {"spheres_plain": [1, 2, 3], "spheres_checker": [1, 2, 3], "spheres_tex": [1, 2, 3], "general_plain": [1, 2, 3, 4, 5],
         "general_tex": [1, 2, 3, 4, 5], "media_many": [1, 2, 3], "limits": sg.LIMIT_SEEDS}
CASES = [(r, s) for r in sg.RECIPES for s in SEEDS[r]]
# one seed per recipe for the heavier GPU tests; general_plain/1: a sphere-bounded and a quad-bounded medium, general_tex/4: a
# negative-radius sphere and an instanced box as boundaries of textured media (test_what_the_recipes_promise asserts both);
# limits: 65 leaves, one a quad
ONE_SEED = {"spheres_plain": 1, "spheres_checker": 2, "spheres_tex": 3, "general_plain": 1, "general_tex": 4, "media_many": 1, "limits": 17}
# the schedule test (the tier kernel and the tail hand-off) also takes these: a box-bounded medium, a negative-radius and an
# instanced boundary in the flat-colour family, a sphere-bounded textured medium
SCHEDULE_EXTRA = [("general_plain", 2), ("general_plain", 4), ("general_tex", 1)]
NX, NY, NS = 48, 32, 4
# the schedule test's frame: 64 tiles of 8 x 8 pixels, the fewest rt_render's cost-aware schedule (and with it the tail hand-off) takes
SCHEDULE_FRAME = (64, 64)
LIVE = [(r, s, NX, NY) for r, s in CASES] + [(r, ONE_SEED[r]) + SCHEDULE_FRAME for r in sg.RECIPES] + [c + SCHEDULE_FRAME for c in SCHEDULE_EXTRA]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("name", NAMED)
def test_description_oracle_equals_named_oracle(art, orc, name):
    """from_desc(HostScene(name).desc) against OracleScene(name): frame bit for bit, all eight counters, the tree, and the
    closest hit of a few thousand rays of the named oracle's own render (t, point, normal, uv bit for bit; the material through
    the index map: the named oracle numbers materials in creation order, the description in the flattener's)."""
    crowd = name.startswith("crowd")
    nx, ny, ns = (16, 16, 1) if crowd else (32, 24, 3)
    img, iw, ih = art.default_texture(name)
    hs = art.HostScene(name, nx, ny, img, iw, ih)
    named = orc.OracleScene(name, nx, ny, img, iw, ih)
    desc = orc.OracleScene.from_desc(hs.desc, nx, ny, hs.gamma, hs.background, hs.use_gradient_bg)
    assert (desc.gamma, desc.gradient) == (named.gamma, named.gradient) and np.array_equal(desc.background, named.background)
    fa, ca = named.render(ns)
    fb, cb = desc.render(ns)
    assert ca == cb
    assert np.array_equal(_bits(fa), _bits(fb))
    # the tree: boxes bit for bit in pre-order, the same nodes are leaves; the named oracle numbers a leaf by its object's
    # creation order (HostScene.leaf_order, tests/test_host_scene.py), the description oracle by its position
    na, nb = named.nodes(), desc.nodes()
    assert na.shape == nb.shape == (hs.desc.n_nodes, 8)
    assert np.array_equal(_bits(na[:, :6]), _bits(nb[:, :6]))
    leaf = nb[:, 6] >= 0
    assert np.array_equal(na[:, 6] >= 0, leaf) and np.array_equal(leaf, hs.nodes()["prim"] >= 0)
    assert np.array_equal(nb[leaf, 6], np.arange(int(leaf.sum())))
    assert np.array_equal(na[:, 6].astype(np.int32), hs.leaf_order())
    # rays
    rays = tf.ray_sample(orc, named, nx, ny, ns)[:4000]
    assert len(rays) >= (400 if crowd else 3000)
    ra = named.trace(rays[:, 0:3], rays[:, 3:6], rays[:, 6])
    rb = desc.trace(rays[:, 0:3], rays[:, 3:6], rays[:, 6])
    for a, b, what in zip(ra[:4], rb[:4], "t p n uv".split()):
        assert np.array_equal(_bits(a), _bits(b)), what
    assert np.array_equal(_bits(rb[0]), _bits(rays[:, 7]))
    pairs = set(zip(ra[4].tolist(), rb[4].tolist()))
    assert len({a for a, _ in pairs}) == len(pairs) == len({b for _, b in pairs}), "the material index map is not one to one"
    assert (-1, -1) in pairs or (ra[4] >= 0).all()
    hit = rb[4] >= 0
    assert (rb[4][hit] < hs.desc.n_materials).all()
    # node_passes() works on a description scene as on a named one
    pa, pb = named.node_passes(1, threads=2), desc.node_passes(1, threads=2)
    assert np.array_equal(pa[0], pb[0]) and pa[1:] == pb[1:]


def test_non_binary_tree_is_refused(art, orc):
    """An interior node with three children, or with one, is refused: the oracle's bvh_hit is binary."""
    hs = art.HostScene("cornell", 16, 16)
    assert orc.OracleScene.from_desc(hs.desc, 16, 16).h >= 0

    def refused(nodes):
        d = art.RtSceneDesc.from_buffer_copy(hs.desc)
        d.nodes, d.n_nodes = nodes.ctypes.data, len(nodes)
        with pytest.raises(ValueError):
            orc.OracleScene.from_desc(d, 16, 16)

    n = hs.nodes()
    leaves = n[n["prim"] >= 0][:3]
    three = np.zeros(4, art.NODE_DTYPE)           # a root over three leaves: a legal walk array, not a binary tree
    three[0] = (leaves["bmin"].min(0), 4, leaves["bmax"].max(0), -1)
    three[1:] = leaves
    three["skip"][1:] = [2, 3, 4]
    refused(three)
    one = three[:2].copy()                        # a root over a single leaf
    one["skip"] = [2, 2]
    refused(one)
    inner = n.copy()                              # the first interior node below the root loses its second child's link
    k = int(np.flatnonzero(inner["prim"] < 0)[1])
    inner["skip"][k + 1] = inner["skip"][k]
    refused(inner)
    # and the product takes the three-leaf root: any hierarchy over the leaves is a legal description (checked on the GPU)


def test_generator_is_deterministic_and_well_formed():
    for recipe, seed in CASES:
        a, b = sg.generate(recipe, seed), sg.generate(recipe, seed)
        n = a.nodes()
        assert np.array_equal(n, b.nodes()) and np.array_equal(a.spheres(), b.spheres()) and np.array_equal(a.textures(), b.textures())
        assert a.n_leaves <= (200 if recipe != "limits" else 65) and len(n) == 2 * a.n_leaves - 1
        idx = np.arange(len(n))
        assert (n["skip"] > idx).all() and (n["skip"] <= len(n)).all() and n["skip"][0] == len(n)
        for i in np.flatnonzero(n["prim"] < 0):   # an interior box is exactly the union of its two children's
            c1 = i + 1
            c2 = n["skip"][c1]
            assert n["skip"][c2] == n["skip"][i]
            assert np.array_equal(n["bmin"][i], np.minimum(n["bmin"][c1], n["bmin"][c2]))
            assert np.array_equal(n["bmax"][i], np.maximum(n["bmax"][c1], n["bmax"][c2]))
        if recipe == "limits":
            assert a.n_leaves == sg.LIMIT_COUNTS[seed % 9] and a.desc.n_quads == (1 if seed >= 9 else 0)
    trees = {tuple(sg.generate("spheres_plain", s).nodes()["skip"][:8]) for s in (1, 2, 3)}
    assert len(trees) == 3                        # the split points come from the seed
    assert {sg.generate(r, ONE_SEED[r]).has_tier_data for r in sg.RECIPES} == {True, False}
    assert not sg.generate("media_many", ONE_SEED["media_many"]).has_tier_data


def test_what_the_recipes_promise():
    """The things no named scene contains are in the generated ones (read from the arrays, not from the recipe's text)."""
    seen = {"ior": set(), "octaves": set(), "flags": set(), "uvoff_over": set(), "checker_over": set(), "boundary": set(), "n_media": set(),
            "inst_child": set(), "levels": set()}
    for recipe, seed in CASES:
        g = sg.generate(recipe, seed)
        m, t, ins, med, sph = g.materials(), g.textures(), g.instances(), g.media(), g.spheres()
        cam = g.desc.camera
        seen["ior"] |= {round(float(x), 2) for x in m["ior"][m["kind"] == sg.DIELECTRIC]}
        seen["octaves"] |= set(t["a"][t["kind"] == sg.T_NOODLE].tolist())
        seen["flags"] |= set(ins["flags"].tolist())
        seen["uvoff_over"] |= set(t["kind"][t["a"][t["kind"] == sg.T_UVOFF]].tolist())
        for c in t[t["kind"] == sg.T_CHECKER]:
            seen["checker_over"] |= {int(t["kind"][c["a"]]), int(t["kind"][c["b"]])}
        seen["boundary"] |= set((med["boundary"] >> 28).tolist())
        seen["inst_child"] |= set((ins["child"] >> 28).tolist())
        seen["n_media"].add(len(med))
        assert (m["tex"][m["kind"] == sg.LIGHT] < 0).all()                          # lights are solid-coloured
        if len(med) and recipe != "limits":
            assert cam.lens_radius > 0                                              # a lens together with instances or media
        if recipe in ("general_plain", "general_tex", "media_many"):
            assert (cam.time0, cam.time1) == (0.25, 0.75)
        if recipe in ("general_tex",) and len(med):
            seen["levels"].add(("medium_tex", bool((m["tex"][med["mat"]] >= 0).any())))
        if recipe == "general_plain":
            assert set(t["kind"].tolist()) <= {sg.T_SOLID, sg.T_CHECKER}
        if len(ins):
            shells = sph["radius"][(ins["child"][(ins["child"] >> 28) == sg.SPHERE]) & 0x0FFFFFFF]
            seen["shell_under_instance"] = seen.get("shell_under_instance", False) or bool((shells < 0).any())
    assert {0.67, 1.0, 1.5, 2.4} <= seen["ior"], seen
    assert {0, 1, 16} <= seen["octaves"], seen
    assert {1, 2, 3} <= seen["flags"], seen
    assert {sg.T_IMAGE, sg.T_SOLID, sg.T_NOISE, sg.T_NOODLE, sg.T_FELT} <= seen["uvoff_over"], seen
    assert {sg.T_NOISE, sg.T_IMAGE, sg.T_SOLID} <= seen["checker_over"], seen
    assert {sg.SPHERE, sg.QUAD, sg.BOX, sg.INSTANCE} <= seen["boundary"], seen
    assert {sg.SPHERE, sg.QUAD, sg.BOX} <= seen["inst_child"], seen
    assert {0, 1, 2, 3} <= seen["n_media"] and max(seen["n_media"]) <= 5, seen
    assert seen["shell_under_instance"] and ("medium_tex", True) in seen["levels"], seen


def _media_of(g):
    """Per medium of a generated scene: (boundary kind, the boundary sphere's radius or None, kind of an instanced boundary's
    child or None, whether the isotropic material is textured) -- read from the arrays."""
    med, sph, ins, m = g.media(), g.spheres(), g.instances(), g.materials()
    out = []
    for x in med:
        kind, idx = int(x["boundary"]) >> 28, int(x["boundary"]) & 0x0FFFFFFF
        child = int(ins["child"][idx]) >> 28 if kind == sg.INSTANCE else None
        out.append((kind, float(sph["radius"][idx]) if kind == sg.SPHERE else None, child, bool(m["tex"][x["mat"]] >= 0)))
    return out


@pytest.mark.parametrize("recipe", ["general_plain", "general_tex"])
def test_general_recipes_hold_every_medium_boundary(recipe):
    """Within each general recipe's own seed list: 0, 1 and 2 media; a boundary of each kind -- sphere, negative-radius sphere,
    quad, box, instance (of a box and of a sphere); in general_tex textured isotropic materials.  The seeds behind the heavier
    GPU tests (ONE_SEED, SCHEDULE_EXTRA) have media that enclose a volume, and instances with every combination of flags."""
    per_seed = {s: _media_of(sg.generate(recipe, s)) for s in SEEDS[recipe]}
    media = [x for v in per_seed.values() for x in v]
    assert {len(v) for v in per_seed.values()} == {0, 1, 2}, per_seed
    assert {k for k, _, _, _ in media} == {sg.SPHERE, sg.QUAD, sg.BOX, sg.INSTANCE}, per_seed
    radii = [r for k, r, _, _ in media if k == sg.SPHERE]
    assert min(radii) < 0 < max(radii), radii
    assert {c for k, _, c, _ in media if k == sg.INSTANCE} == {sg.SPHERE, sg.BOX}, per_seed
    if recipe == "general_tex":
        assert any(t for _, _, _, t in media), per_seed
    for r, s in [(recipe, ONE_SEED[recipe])] + [c for c in SCHEDULE_EXTRA if c[0] == recipe]:
        g = sg.generate(r, s)
        mine = _media_of(g)
        assert any(k != sg.QUAD for k, _, _, _ in mine), (s, mine)           # (a single quad encloses nothing and never scatters)
        assert set(g.instances()["flags"].tolist()) == {1, 2, 3} and g.desc.n_boxes > 0
    one = _media_of(sg.generate(recipe, ONE_SEED[recipe]))
    if recipe == "general_tex":                                              # a textured medium inside a negative-radius boundary
        assert any(k == sg.SPHERE and r < 0 and t for k, r, _, t in one), one
    else:
        assert {k for k, _, _, _ in one} == {sg.SPHERE, sg.QUAD}, one
    # what the tier kernel meets in the flat-colour family (the schedule test): sphere, negative sphere, box, instance boundaries
    sched = [x for r, s in [(recipe, ONE_SEED[recipe])] + SCHEDULE_EXTRA if r == "general_plain" for x in _media_of(sg.generate(r, s))]
    if recipe == "general_plain":
        assert {sg.SPHERE, sg.BOX, sg.INSTANCE} <= {k for k, _, _, _ in sched} and any(r is not None and r < 0 for _, r, _, _ in sched), sched


def test_media_many_boundaries():
    for s in SEEDS["media_many"]:
        g = sg.generate("media_many", s)
        mine = _media_of(g)
        assert 3 <= len(mine) <= 5 and (sg.INSTANCE, None, sg.SPHERE, False) in mine
        assert not g.has_tier_data
    assert {len(_media_of(sg.generate("media_many", s))) for s in SEEDS["media_many"]} >= {3}


@pytest.fixture(scope="module")
def empty_frames(orc):
    cache = {}

    def get(g):
        key = (bytes(g.desc.camera), g.nx, g.ny, g.use_gradient_bg, tuple(g.background))
        if key not in cache:
            cache[key] = orc.OracleScene.from_host(g.emptied()).render(NS, counters=False)[0]
        return cache[key]
    return get


@pytest.mark.parametrize("recipe,seed,nx,ny", LIVE)
def test_generated_scene_is_live(orc, empty_frames, recipe, seed, nx, ny):
    """Conditions on the inputs of the GPU tests, from the oracle alone: a scene every ray misses would test nothing.  Every
    counter the scene's contents imply is non-zero, at least 1.3 rays per sample, and at least half the pixels differ from the
    same camera's frame with no objects.  If a seed fails, the generator's placement is what changes -- not these numbers."""
    g = sg.generate(recipe, seed, nx, ny)
    assert (g.nx, g.ny, g.ns) == (nx, ny, NS)
    fb, cnt = orc.OracleScene.from_host(g).render(NS)
    assert not np.isnan(fb).any()
    implied = set(g.contents)
    d = g.desc
    assert implied == {k for k, n in (("sphere_tests", d.n_spheres), ("quad_tests", d.n_quads), ("box6_calls", d.n_boxes),
                                      ("inst_calls", d.n_instances), ("medium_calls", d.n_media)) if n}
    for k in implied:
        assert cnt[k] > 0, (k, cnt)
    assert cnt["samples"] == nx * ny * NS and cnt["rays"] >= 1.3 * cnt["samples"], cnt
    differ = (_bits(fb) != _bits(empty_frames(g))).any(axis=-1)
    assert differ.mean() >= 0.5, float(differ.mean())


def test_empty_description(orc):
    """n_nodes = 0: an empty world.  Every ray misses: one ray per sample, each against the root's empty box and nothing else;
    the frame is the background."""
    g = sg.generate("spheres_plain", 1).emptied()
    o = orc.OracleScene.from_host(g)
    fb, cnt = o.render(2, gamma=1.0)
    assert cnt["rays"] == cnt["samples"] == cnt["box_tests"] == NX * NY * 2
    assert all(cnt[k] == 0 for k in ("sphere_tests", "quad_tests", "medium_calls", "box6_calls", "inst_calls"))
    assert len(o.nodes()) == 1 and o.nodes()[0, 6] == -1
    assert (fb > 0).all() and (fb <= 1).all()
    t, p, n, uv, mat = o.trace(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))
    assert (t == tf.FLT_MAX).all() and (mat == -1).all()
