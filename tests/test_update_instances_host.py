"""rt_refit_instances, the host-only statement of what rt_scene_update_instances is equivalent to (include/rt_abi.h), against the
NumPy restatement tests/refit_instances_expect.py on generated and named scenes; the rule against the host flattener's own
boxes; its refusals; and the rule's boxes checked through the CPU oracle.  No GPU involved."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import refit_instances_expect as ri
import scene_gen as sg

NX, NY, NS, SEED = 48, 32, 4, 1984
# general_plain 0: every instance kind, a child shared by several instances; 4: a medium bounded by an instanced box; 5: one bounded
# by an instanced moving sphere.  scene_gen's `limits` recipe holds no instance at any seed (the selection below is empty and
# asserted so), so its leaf counts -- 1, 2, 12, 13, 24, 25, 63, 64, 65 -- come from ri.small_scene, which is `limits` with instances
LIMITS_WITH_INSTANCES = [s for s in sg.LIMIT_SEEDS if len(sg.generate("limits", s, NX, NY).instances())]
SCENES = [("general_plain", 0), ("general_plain", 4), ("general_plain", 5)] + [("limits", s) for s in LIMITS_WITH_INSTANCES] + \
         [("small", n) for n in sg.LIMIT_COUNTS]
NAMED = ["instanced", "cornell", "cornell_smoke", "fog", "crowd_big"]
_scenes = {}


def _scene(recipe, seed):
    if (recipe, seed) not in _scenes:
        _scenes[(recipe, seed)] = ri.small_scene(seed, 0, NX, NY) if recipe == "small" else sg.generate(recipe, seed, NX, NY)
    return _scenes[(recipe, seed)]


def _check_against_restatement(art, scene, idx, rec, what):
    got_nodes, got_inst = art.refit_instances(scene.desc, rec, idx)
    want_nodes, want_inst, _, _ = ri.refit(scene, idx, rec)
    base = scene.nodes()
    assert np.array_equal(got_nodes["skip"], base["skip"]) and np.array_equal(got_nodes["prim"], base["prim"]), what
    ri.same_values(got_nodes["bmin"], want_nodes["bmin"], what + " bmin")
    ri.same_values(got_nodes["bmax"], want_nodes["bmax"], what + " bmax")
    assert got_inst.tobytes() == want_inst.tobytes(), what
    return got_nodes, got_inst


def test_limits_recipe_holds_no_instance():
    assert LIMITS_WITH_INSTANCES == []
    for n in sg.LIMIT_COUNTS:
        scene = _scene("small", n)
        assert scene.n_leaves == n and len(ri.followed(scene)) >= 1


def test_symbols_and_layout(art, tmp_path):
    for sym in ("rt_scene_update_instances", "rt_scene_get_instances", "rt_refit_instances", "rt_multi_update_instances"):
        assert sym in art.RT_ABI_SYMBOLS and hasattr(art.rt_lib(), sym)
    fields = [f for f, _ in art.RtInstanceUpdate._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\", sizeof(rt_instance_update));\n"
                   + "".join(f"  printf(\" %zu\", offsetof(rt_instance_update, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", f"{art.REPO_ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(art.RtInstanceUpdate) == 24
    assert out[1:] == [getattr(art.RtInstanceUpdate, f).offset for f in fields]


def test_the_restatements_fma_rounds_once():
    """fma32 against exact rational arithmetic, on operands that cancel (where a double-rounded sum goes wrong) and on plain ones."""
    rng = np.random.default_rng(3)
    a = rng.uniform(-1, 1, 4000).astype(np.float32)
    x = rng.uniform(-600, 600, 4000).astype(np.float32)
    b = np.where(rng.integers(2, size=4000) == 0, -(a * x) * (1 + rng.uniform(-1e-6, 1e-6, 4000)), rng.uniform(-600, 600, 4000)).astype(np.float32)
    r = ri.fma32(a, x, b)
    assert all(ri.is_correctly_rounded_fma(a[k], x[k], b[k], r[k]) for k in range(len(a)))
    assert (r != (a * x + b)).any()                                   # the unfused float32 form differs somewhere


def test_instance_record_uses_the_references_arithmetic(art):
    hs = art.HostScene("cornell", NX, NY)
    inst = hs.instances()
    assert len(inst) == 2 and (inst["flags"] == 3).all()
    made = set()
    for k in range(2):                                                # the two blocks of the Cornell box: rotate_y by 15 and by -18 degrees
        for deg in (15.0, -18.0):
            if art.instance_record(int(inst["child"][k]), deg, inst["offset"][k]).tobytes() == inst[k:k + 1].tobytes():
                made.add(deg)
    assert made == {15.0, -18.0}, (made, inst)
    assert int(art.instance_record(5, None, (1, 2, 3))["flags"][0]) == 2 and int(art.instance_record(5, 10.0)["flags"][0]) == 1
    with pytest.raises(ValueError):
        art.instance_record(5)
    hs.close()


@pytest.mark.parametrize("kind", ri.UPDATES)
@pytest.mark.parametrize("recipe,seed", SCENES)
def test_refit_instances_equals_the_restatement(art, recipe, seed, kind):
    scene = _scene(recipe, seed)
    inst = scene.instances()
    idx, rec = ri.make_update(scene, kind)
    got_nodes, _ = _check_against_restatement(art, scene, idx, rec, f"{scene.name} {kind}")
    base = scene.nodes()
    for i in np.flatnonzero(base["prim"] < 0):                        # interior boxes contain their children
        j = i + 1
        while j < base["skip"][i]:
            assert (got_nodes["bmin"][i] <= got_nodes["bmin"][j]).all() and (got_nodes["bmax"][i] >= got_nodes["bmax"][j]).all(), (scene.name, kind, i, j)
            j = base["skip"][j]
    leaf = base["prim"] >= 0                                          # leaves no update follows are untouched
    li = ri.leaf_instances(base["prim"][leaf], scene.media(), len(inst))
    keep = np.flatnonzero(leaf)[~np.isin(li, idx)]
    assert got_nodes[keep].tobytes() == base[keep].tobytes()
    if kind == "far" and len(base) > 1:                               # the root grew
        assert got_nodes["bmax"][0][0] > base["bmax"][0][0] + 100 and got_nodes["bmin"][0][2] < base["bmin"][0][2] - 100


@pytest.mark.parametrize("recipe,seed", SCENES)
def test_moving_back_restores_the_rule_boxes(art, recipe, seed):
    """far, then back: the second update runs on D' of the first; the root shrinks again and every box equals the restatement's."""
    scene = _scene(recipe, seed)
    idx, rec = ri.make_update(scene, "far")
    far = ri.moved_scene(scene, idx, rec)
    back = scene.instances()[idx]
    got, _ = _check_against_restatement(art, far, idx, back, f"{scene.name} back")
    direct, _, _, _ = ri.refit(scene, idx, back)
    ri.same_values(got["bmin"], direct["bmin"], "back == the update applied to the original")
    ri.same_values(got["bmax"], direct["bmax"], "back == the update applied to the original")


@pytest.mark.parametrize("name", NAMED)
def test_rule_is_the_host_flatteners(art, name):
    """Every followed instance written back unchanged: no box moves, so the rule gives the host library's boxes value for value."""
    hs = art.HostScene(name, NX, NY)
    idx, rec = ri.make_update(hs, "identity")
    assert len(idx) >= 1
    base = hs.nodes()
    for got, who in ((art.refit_instances(hs.desc, rec, idx)[0], "library"), (ri.refit(hs, idx, rec)[0], "restatement")):
        assert np.array_equal(got["skip"], base["skip"]) and np.array_equal(got["prim"], base["prim"])
        ri.same_values(got["bmin"], base["bmin"], f"{name} {who} bmin")
        ri.same_values(got["bmax"], base["bmax"], f"{name} {who} bmax")
    if name == "cornell_smoke":                                       # both instances are boundaries of media
        assert ((base["prim"][base["prim"] >= 0] >> 28) == sg.MEDIUM).sum() == 2 and len(idx) == 2
    hs.close()


def test_refusals_name_the_check_and_write_nothing(art):
    scene = _scene("general_plain", 0)
    L = art.rt_lib()
    inst = scene.instances()
    ids = ri.followed(scene)
    nodes_out, inst_out = np.full(len(scene.nodes()), 7, np.uint8).repeat(32), np.full(len(inst), 7, np.uint8).repeat(32)

    def refused(why, rec, idx=None, first=0, count=None, on=scene):
        u = art.RtInstanceUpdate()
        rec = np.ascontiguousarray(rec)
        u.count, u.first = len(rec) if count is None else count, first
        u.instances = rec.ctypes.data if len(rec) else None
        keep = None if idx is None else np.ascontiguousarray(idx, np.int32)
        u.indices = None if keep is None else keep.ctypes.data
        assert L.rt_refit_instances(C.byref(on.desc), C.byref(u), nodes_out.ctypes.data, inst_out.ctypes.data) == 1
        assert L.rt_last_error_detail().decode() == why
        assert (nodes_out == 7).all() and (inst_out == 7).all()

    NON_FINITE, FLAGS = "rt_refit_instances: an instance record has a non-finite sin_t, cos_t or offset", "rt_refit_instances: instance flags must be 1, 2 or 3"
    CHILD = "rt_refit_instances: an instance record's child is not the child the scene holds (the child of an instance cannot change)"
    RANGE, TWICE = "rt_refit_instances: instance index out of range", "rt_refit_instances: an instance index appears twice"
    MORE = "rt_refit_instances: more records than the scene has instances (an index is out of range or appears twice)"
    one = inst[ids[:1]]
    assert L.rt_refit_instances(C.byref(scene.desc), None, nodes_out.ctypes.data, inst_out.ctypes.data) == 1
    assert L.rt_last_error_detail().decode() == "rt_refit_instances: null update"
    assert L.rt_refit_instances(None, None, None, None) == 1
    refused("rt_refit_instances: count is negative", one, count=-1)
    refused("rt_refit_instances: null instance records", inst[:0], count=1)
    refused(RANGE, one, idx=[len(inst)])
    refused(RANGE, one, idx=[-1])
    refused(RANGE, inst[:2], first=len(inst) - 1)
    refused(TWICE, inst[ids[[0, 1, 0]]], idx=ids[[0, 1, 0]])
    for field, value in (("sin_t", np.nan), ("cos_t", np.inf), ("offset", -np.inf)):
        bad = one.copy()
        bad[field] = value
        refused(NON_FINITE, bad, idx=ids[:1])
    for flags in (0, 4, -1):
        bad = one.copy()
        bad["flags"] = flags
        refused(FLAGS, bad, idx=ids[:1])
    # two faults at once, on three instances: records are looked at after every index has passed, the count before any index
    tiny = sg.tiny()
    few = tiny.instances()
    assert len(few) == 3 and len(set(few["child"])) == 3
    for field, value in (("sin_t", np.nan), ("flags", 0), ("child", few["child"][2])):
        bad = few[[0, 1]]
        bad[field][0] = value
        refused(RANGE, bad, idx=[0, 3], on=tiny)                      # record 0 is bad, index 1 is out of range
        bad = few[[0, 1, 0]]
        bad[field][1] = value
        refused(TWICE, bad, idx=[0, 1, 0], on=tiny)                   # record 1 is bad, index 0 comes again as index 2
    refused(MORE, few[[0, 0, 1, 2]], idx=[3, 0, 1, 2], on=tiny)       # too many records, index 0 is out of range
    bad = one.copy()
    bad["child"] = inst["child"][ids[1]] if inst["child"][ids[1]] != one["child"][0] else inst["child"][ids[2]]
    assert bad["child"][0] != one["child"][0]
    refused(CHILD, bad, idx=ids[:1])
    with pytest.raises(ValueError, match="child"):
        art.refit_instances(scene.desc, bad, ids[:1])
    with pytest.raises(ValueError, match="INSTANCE_DTYPE"):
        art.refit_instances(scene.desc, np.zeros((1, 8), np.float32))
    with pytest.raises(ValueError, match="one per record"):
        art.refit_instances(scene.desc, one, [0, 1])
    ok = one.copy()
    ok["pad"] = 12345                                                 # pad is not looked at, and kept
    _, out = art.refit_instances(scene.desc, ok, ids[:1])
    assert out[ids[0]]["pad"] == 12345
    # count == 0 is a successful no-op: the description comes back as it is
    nodes, out = art.refit_instances(scene.desc, inst[:0])
    assert nodes.tobytes() == scene.nodes().tobytes() and out.tobytes() == inst.tobytes()


@pytest.mark.parametrize("recipe,seed", [("general_plain", 0), ("general_plain", 4), ("small", 25)])
def test_rule_boxes_contain_their_instances_by_the_oracle(art, orc, recipe, seed):
    """A box that cut into its object would lose hits.  The oracle's frame of D' differs from the unmoved frame and equals, in
    every pixel and in its ray count, its frame of the same tree and records with every instance-following leaf boxed 12 units
    wider on every side -- more than the scene's extent, so that box holds the instance wherever a wrong rule could have put
    the rule's box: the instance alone is hit exactly where it is hit under the rule's box."""
    scene = _scene(recipe, seed)
    idx, rec = ri.make_update(scene, "all")
    nodes, inst = art.refit_instances(scene.desc, rec, idx)
    moved = ri.Moved(scene, nodes, inst)
    first, _ = orc.OracleScene.from_host(scene, NX, NY).render(NS, seed_base=SEED)
    ruled, cnt = orc.OracleScene.from_host(moved, NX, NY).render(NS, seed_base=SEED)
    assert not np.array_equal(ruled, first)
    # the same tree with every followed leaf's box blown up to hold anything the instance could be: equal frames, equal rays
    base = scene.nodes()
    leaf = np.flatnonzero(base["prim"] >= 0)
    li = ri.leaf_instances(base["prim"][leaf], scene.media(), len(inst))
    lo, hi = nodes["bmin"][leaf].copy(), nodes["bmax"][leaf].copy()
    lo[li >= 0] -= np.float32(12.0)
    hi[li >= 0] += np.float32(12.0)
    roomy = ri.Moved(scene, ri.refit_array(base, lo, hi), inst)
    outward, cnt2 = orc.OracleScene.from_host(roomy, NX, NY).render(NS, seed_base=SEED)
    differing = int((ruled.view(np.uint32) != outward.view(np.uint32)).any(-1).sum())
    assert differing == 0 and cnt["rays"] == cnt2["rays"], (differing, cnt["rays"], cnt2["rays"])
