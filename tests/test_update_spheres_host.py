"""rt_refit_nodes, the host-only statement of what rt_scene_update_spheres is equivalent to (include/rt_abi.h), against the NumPy
restatement tests/refit_expect.py on generated and named scenes; its refusals; and the box rule itself, checked through the CPU
oracle against the generator's outward-rounded boxes.  No GPU involved."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import refit_expect as rf
import scene_gen as sg

NX, NY, NS, SEED = 48, 32, 4, 1984
# spheres-only seeds; general_plain seeds whose media are bounded by a sphere (GENERAL_MEDIA: seed 0 and 1 hold kind 0, seed 4 kind 1,
# the negative-radius sphere); media_many (no tier data); limits seeds of 1, 2, 63, 64 and 65 leaves
SCENES = [("spheres_plain", 0), ("spheres_plain", 1), ("spheres_plain", 5), ("general_plain", 0), ("general_plain", 1), ("general_plain", 4),
          ("media_many", 0), ("limits", 0), ("limits", 1), ("limits", 6), ("limits", 7), ("limits", 8)]
UPDATES = rf.UPDATES
make_update = rf.make_update
_scenes = {}


def _scene(recipe, seed):
    if (recipe, seed) not in _scenes:
        _scenes[(recipe, seed)] = sg.generate(recipe, seed, NX, NY)
    return _scenes[(recipe, seed)]


def _check_against_restatement(art, scene, idx, rec, what):
    got_nodes, got_spheres = art.refit_nodes(scene.desc, rec, idx)
    want_nodes, want_spheres, _, _ = rf.refit(scene, idx, rec)
    base = scene.nodes()
    assert np.array_equal(got_nodes["skip"], base["skip"]) and np.array_equal(got_nodes["prim"], base["prim"]), what
    rf.same_values(got_nodes["bmin"], want_nodes["bmin"], what + " bmin")
    rf.same_values(got_nodes["bmax"], want_nodes["bmax"], what + " bmax")
    assert got_spheres.tobytes() == want_spheres.tobytes(), what
    return got_nodes, got_spheres


def test_symbols_and_layout(art, tmp_path):
    for sym in ("rt_scene_update_spheres", "rt_scene_get_spheres", "rt_multi_update_spheres", "rt_refit_nodes", "rt_debug_scene_boxes"):
        assert sym in art.RT_ABI_SYMBOLS and hasattr(art.rt_lib(), sym)
    fields = [f for f, _ in art.RtSphereUpdate._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\", sizeof(rt_sphere_update));\n"
                   + "".join(f"  printf(\" %zu\", offsetof(rt_sphere_update, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", f"{art.REPO_ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(art.RtSphereUpdate) == 24
    assert out[1:] == [getattr(art.RtSphereUpdate, f).offset for f in fields]


@pytest.mark.parametrize("kind", UPDATES)
@pytest.mark.parametrize("recipe,seed", SCENES)
def test_refit_nodes_equals_the_restatement(art, recipe, seed, kind):
    scene = _scene(recipe, seed)
    idx, rec = make_update(scene, kind)
    got_nodes, _ = _check_against_restatement(art, scene, idx, rec, f"{scene.name} {kind}")
    base = scene.nodes()
    # interior boxes contain their children; leaves no update follows are untouched
    for i in np.flatnonzero(base["prim"] < 0):
        j = i + 1
        while j < base["skip"][i]:
            assert (got_nodes["bmin"][i] <= got_nodes["bmin"][j]).all() and (got_nodes["bmax"][i] >= got_nodes["bmax"][j]).all(), (scene.name, kind, i, j)
            j = base["skip"][j]
    leaf = base["prim"] >= 0
    ls = rf.leaf_spheres(base["prim"][leaf], scene.media(), len(scene.spheres()))
    keep = np.flatnonzero(leaf)[~np.isin(ls, idx)]
    assert got_nodes[keep].tobytes() == base[keep].tobytes()
    if kind == "far" and len(base) > 1:                               # the root grew
        assert got_nodes["bmax"][0][0] > base["bmax"][0][0] + 100 and got_nodes["bmin"][0][2] < base["bmin"][0][2] - 100


@pytest.mark.parametrize("recipe,seed", SCENES)
def test_moving_back_restores_the_rule_boxes(art, recipe, seed):
    """far, then back: the second update runs on D' of the first; the root shrinks again and every box equals the restatement's."""
    scene = _scene(recipe, seed)
    idx, rec = make_update(scene, "far")
    far = rf.moved_scene(scene, idx, rec)
    back = scene.spheres()[idx]
    got, _ = _check_against_restatement(art, far, idx, back, f"{scene.name} back")
    direct, _, _, _ = rf.refit(scene, idx, back)
    rf.same_values(got["bmin"], direct["bmin"], "back == the update applied to the original")
    rf.same_values(got["bmax"], direct["bmax"], "back == the update applied to the original")


@pytest.mark.parametrize("name", ["random_scene", "book1"])
def test_rule_is_the_host_flatteners(art, name):
    """Every sphere written back unchanged: no box moves, so the rule gives the host library's sphere boxes value for value."""
    hs = art.HostScene(name, NX, NY)
    sph, base = hs.spheres(), hs.nodes()
    assert len(rf.direct_spheres(hs)) == len(sph) > 100
    nodes, out = art.refit_nodes(hs.desc, sph)
    assert out.tobytes() == sph.tobytes()
    assert np.array_equal(nodes["skip"], base["skip"]) and np.array_equal(nodes["prim"], base["prim"])
    rf.same_values(nodes["bmin"], base["bmin"], name)
    rf.same_values(nodes["bmax"], base["bmax"], name)
    if name == "random_scene":
        assert (sph["vel"] != 0).any()                               # moving spheres among them
    hs.close()


def test_refusals_name_the_check_and_write_nothing(art):
    scene = _scene("general_plain", 0)
    L = art.rt_lib()
    sph = scene.spheres()
    direct = rf.direct_spheres(scene)
    under = np.flatnonzero(rf.instanced(scene.instances(), len(sph)))
    assert len(under) > 0
    nodes_out, sph_out = np.full(len(scene.nodes()), 7, np.uint8).repeat(32), np.full(len(sph), 7, np.uint8).repeat(32)

    def refused(why, rec, idx=None, first=0, count=None, on=scene):
        u = art.RtSphereUpdate()
        rec = np.ascontiguousarray(rec)
        u.count, u.first = len(rec) if count is None else count, first
        u.spheres = rec.ctypes.data if len(rec) else None
        keep = None if idx is None else np.ascontiguousarray(idx, np.int32)
        u.indices = None if keep is None else keep.ctypes.data
        assert L.rt_refit_nodes(C.byref(on.desc), C.byref(u), nodes_out.ctypes.data, sph_out.ctypes.data) == 1
        assert L.rt_last_error_detail().decode() == why
        assert (nodes_out == 7).all() and (sph_out == 7).all()

    NON_FINITE = "rt_refit_nodes: a sphere record has a non-finite c0, vel or radius"
    RANGE, TWICE, MATERIAL = "rt_refit_nodes: sphere index out of range", "rt_refit_nodes: a sphere index appears twice", "rt_refit_nodes: sphere material out of range"
    MORE = "rt_refit_nodes: more records than the scene has spheres (an index is out of range or appears twice)"
    INSTANCED = "rt_refit_nodes: an updated sphere is the child of an instance (its box follows the instance's rule)"
    one = sph[direct[:1]]
    assert L.rt_refit_nodes(C.byref(scene.desc), None, nodes_out.ctypes.data, sph_out.ctypes.data) == 1
    assert L.rt_last_error_detail().decode() == "rt_refit_nodes: null update"
    assert L.rt_refit_nodes(None, None, None, None) == 1
    refused("rt_refit_nodes: count is negative", one, count=-1)
    refused("rt_refit_nodes: null sphere records", sph[:0], count=1)
    refused(RANGE, one, idx=[len(sph)])
    refused(RANGE, one, idx=[-1])
    refused(RANGE, sph[:2], first=len(sph) - 1)
    refused(TWICE, sph[direct[[0, 1, 0]]], idx=direct[[0, 1, 0]])
    for field, value in (("c0", np.nan), ("vel", np.inf), ("radius", -np.inf)):
        bad = one.copy()
        bad[field] = value
        refused(NON_FINITE, bad, idx=direct[:1])
    for mat in (-1, len(scene.materials())):
        bad = one.copy()
        bad["mat"] = mat
        refused(MATERIAL, bad, idx=direct[:1])
    refused(INSTANCED, sph[under[:1]], idx=under[:1])
    # two faults at once, on three spheres: a record is looked at as soon as its index has passed, the count before any index
    tiny = sg.tiny()
    few = tiny.spheres()
    assert len(few) == 3
    bad = few[[0, 1]]
    bad["c0"][0] = np.nan
    refused(NON_FINITE, bad, idx=[0, 3], on=tiny)                     # record 0 is bad, index 1 is out of range
    bad = few[[0, 1, 0]]
    bad["vel"][1] = np.nan
    refused(NON_FINITE, bad, idx=[0, 1, 0], on=tiny)                  # record 1 is bad, index 0 comes again as index 2
    refused(MORE, few[[0, 0, 1, 2]], idx=[3, 0, 1, 2], on=tiny)       # too many records, index 0 is out of range
    with pytest.raises(ValueError, match="child of an instance"):
        art.refit_nodes(scene.desc, sph[under[:1]], under[:1])
    with pytest.raises(ValueError, match="SPHERE_DTYPE"):
        art.refit_nodes(scene.desc, np.zeros((1, 8), np.float32))
    with pytest.raises(ValueError, match="one per record"):
        art.refit_nodes(scene.desc, one, [0, 1])
    # count == 0 is a successful no-op: the description comes back as it is
    nodes, out = art.refit_nodes(scene.desc, sph[:0])
    assert nodes.tobytes() == scene.nodes().tobytes() and out.tobytes() == sph.tobytes()


@pytest.mark.parametrize("recipe,seed", [("spheres_plain", 1), ("general_plain", 0), ("limits", 8)])
def test_rule_boxes_contain_their_spheres_by_the_oracle(art, orc, recipe, seed):
    """The oracle's frame of D' differs from the unmoved frame and equals, in every pixel, its frame of the same tree with the
    moved spheres boxed by the generator's own outward-rounded rule: a box that cut into its sphere would lose hits."""
    scene = _scene(recipe, seed)
    idx, rec = make_update(scene, "all")
    rec["vel"][::3] = np.array([0.05, 0.3, 0.0], np.float32)         # some of them moving
    first, _ = orc.OracleScene.from_host(scene, NX, NY).render(NS, seed_base=SEED)
    nodes, spheres = art.refit_nodes(scene.desc, rec, idx)
    ruled, cnt = orc.OracleScene.from_host(rf.Moved(scene, nodes, spheres), NX, NY).render(NS, seed_base=SEED)
    outward, cnt2 = orc.OracleScene.from_host(rf.moved_scene(scene, idx, rec, rf.generator_box), NX, NY).render(NS, seed_base=SEED)
    assert not np.array_equal(ruled, first)
    differing = int((ruled.view(np.uint32) != outward.view(np.uint32)).any(-1).sum())
    assert differing == 0 and cnt["rays"] == cnt2["rays"], (differing, cnt["rays"], cnt2["rays"])
