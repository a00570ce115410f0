"""rt_refit_quads, the host-only statement of what rt_scene_update_quads is equivalent to (include/rt_abi.h), against the NumPy
restatement tests/refit_quads_expect.py on generated and named scenes; the rule against the host flattener's own boxes; the
quad and box constructors of the binding; its refusals; and the rule's boxes checked through the CPU oracle.  No GPU involved."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import refit_quads_expect as rq
import scene_gen as sg

NX, NY, NS, SEED = 48, 32, 4, 1984
# general_plain 0..5: direct oblique and axis-aligned quads, boxes in the reference's face order and in a permuted one, one box
# shared by several instances, a quad under an instance, media bounded by a box (0, 2), a quad (1) and an instance of a box (4);
# limits 9..17: the seeds whose one leaf is a quad (1 .. 65 leaves)
GENERAL = [("general_plain", s) for s in range(6)]
LIMITS = [("limits", s) for s in sg.LIMIT_SEEDS if s >= len(sg.LIMIT_COUNTS)]
NAMED = ["cornell", "cornell_smoke", "crowd_big", "quads", "simple_light", "instanced", "fog"]
_scenes = {}


def _scene(recipe, seed):
    if (recipe, seed) not in _scenes:
        _scenes[(recipe, seed)] = sg.generate(recipe, seed, NX, NY)
    return _scenes[(recipe, seed)]


CASES = [(r, s, k) for r, s in GENERAL for k in rq.UPDATES] + [(r, s, k) for r, s in LIMITS for k in ("one", "all", "tilt", "identity")]


def _check_against_restatement(art, scene, idx, rec, what):
    got_nodes, got_quads = art.refit_quads(scene.desc, rec, idx)
    want_nodes, want_quads, _, _ = rq.refit(scene, idx, rec)
    base = scene.nodes()
    assert np.array_equal(got_nodes["skip"], base["skip"]) and np.array_equal(got_nodes["prim"], base["prim"]), what
    rq.same_values(got_nodes["bmin"], want_nodes["bmin"], what + " bmin")
    rq.same_values(got_nodes["bmax"], want_nodes["bmax"], what + " bmax")
    assert got_quads.tobytes() == want_quads.tobytes(), what
    return got_nodes, got_quads


def test_the_generated_scenes_hold_what_the_updates_need():
    for recipe, seed in GENERAL:
        scene = _scene(recipe, seed)
        assert rq.kinds_for(scene) == rq.UPDATES, (seed, rq.kinds_for(scene))
        c = rq.census(scene)
        codes = c["codes"][c["direct_quads"]]
        assert (codes == 0).any() and (codes != 0).any()              # direct oblique and axis-aligned quads
        assert len(c["direct_boxes"]) >= 1 and len(c["inst_boxes"]) >= 1
    inst = _scene("general_plain", 0).instances()
    kinds = inst["child"] >> 28
    shared = [c for c in np.unique(inst["child"][kinds == sg.BOX]) if (inst["child"] == c).sum() > 1]
    assert shared and (kinds == sg.QUAD).any()                        # one box under several instances, a quad under an instance
    canon = [len(rq.census(_scene(r, s))["canonical"]) < len(_scene(r, s).boxes()) for r, s in GENERAL]
    assert any(canon)                                                 # some box is in a permuted face order
    for recipe, seed in LIMITS:
        scene = _scene(recipe, seed)
        assert len(scene.quads()) == 1 and rq.kinds_for(scene) == ["one", "all", "tilt", "identity"]


def test_symbols_and_layout(art, tmp_path):
    for sym in ("rt_scene_update_quads", "rt_scene_get_quads", "rt_refit_quads", "rt_multi_update_quads", "rt_debug_scene_quads"):
        assert sym in art.RT_ABI_SYMBOLS and hasattr(art.rt_lib(), sym)
    for sym in ("rtw_quad_record", "rtw_box_records"):
        assert hasattr(art.host_lib(), sym)
    fields = [f for f, _ in art.RtQuadUpdate._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu %zu\", sizeof(rt_quad_update), sizeof(rt_quad));\n"
                   + "".join(f"  printf(\" %zu\", offsetof(rt_quad_update, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", f"{art.REPO_ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(art.RtQuadUpdate) == 24 and out[1] == art.QUAD_DTYPE.itemsize == 80
    assert out[2:] == [getattr(art.RtQuadUpdate, f).offset for f in fields]


@pytest.mark.parametrize("recipe,seed,kind", CASES)
def test_refit_quads_equals_the_restatement(art, recipe, seed, kind):
    scene = _scene(recipe, seed)
    idx, rec = rq.make_update(scene, kind)
    got_nodes, _ = _check_against_restatement(art, scene, idx, rec, f"{scene.name} {kind}")
    base = scene.nodes()
    for i in np.flatnonzero(base["prim"] < 0):                        # interior boxes contain their children
        j = i + 1
        while j < base["skip"][i]:
            assert (got_nodes["bmin"][i] <= got_nodes["bmin"][j]).all() and (got_nodes["bmax"][i] >= got_nodes["bmax"][j]).all(), (scene.name, kind, i, j)
            j = base["skip"][j]
    leaf = base["prim"] >= 0                                          # leaves that depend on no updated quad are untouched
    moved = np.zeros(len(scene.quads()), bool)
    moved[idx] = True
    solids = rq.leaf_solids(base["prim"][leaf], scene.media())
    dep = np.array([rq.depends(s, moved, rq.scene_boxes(scene), scene.instances()) for s in solids])
    assert dep.any()
    keep = np.flatnonzero(leaf)[~dep]
    assert got_nodes[keep].tobytes() == base[keep].tobytes()
    if kind == "grow":                                                # one box under several instances: every one of those leaves
        first = int(idx[0])
        box = int(np.flatnonzero(rq.scene_boxes(scene) == first)[0])
        users = int((scene.instances()["child"] == sg.ref(sg.BOX, box)).sum())
        assert dep.sum() == users and (users > 1 or seed != 0)
    # the move back runs on D' and gives the update of the original by its own records
    there = rq.moved_scene(scene, idx, rec)
    back = scene.quads()[idx]
    got, _ = _check_against_restatement(art, there, idx, back, f"{scene.name} {kind} back")
    direct, _, _, _ = rq.refit(scene, idx, back)
    rq.same_values(got["bmin"], direct["bmin"], "back == the update applied to the original")
    rq.same_values(got["bmax"], direct["bmax"], "back == the update applied to the original")


def test_the_restatements_marks_follow_tilt_and_shear():
    """The updates that aim at the marks change them, in the restatement's own terms: a code 1..3 -> 0 and one 0 -> 1..3 under
    tilt, bit 30 of one box dropped under shear and back under its reverse."""
    scene = _scene("general_plain", 0)
    quads, boxes = scene.quads(), rq.scene_boxes(scene)
    q0, b0 = rq.device_records(quads, boxes)
    idx, rec = rq.make_update(scene, "tilt")
    q1, b1 = rq.device_records(rq.refit(scene, idx, rec)[1], boxes)
    before, after = q0["pad0"].view(np.int32)[idx], q1["pad0"].view(np.int32)[idx]
    assert sorted(zip(before != 0, after != 0)) == [(False, True), (True, False)] and np.array_equal(b0, b1)
    idx, rec = rq.make_update(scene, "shear")
    q2, b2 = rq.device_records(rq.refit(scene, idx, rec)[1], boxes)
    changed = np.flatnonzero(b2 != b0)
    assert len(changed) == 1 and b0[changed[0]] == (b2[changed[0]] | rq.CANONICAL) and b2[changed[0]] == boxes[changed[0]]
    q3, b3 = rq.device_records(rq.refit(rq.moved_scene(scene, idx, rec), idx, quads[idx])[1], boxes)
    assert np.array_equal(b3, b0) and q3.tobytes() == q0.tobytes()


@pytest.mark.parametrize("name", NAMED)
def test_rule_is_the_host_flatteners(art, name):
    """Every quad written back unchanged: no box moves, so the rules give the host library's boxes value for value -- for direct
    quads and boxes, which no instance update ever recomputed, too."""
    hs = art.HostScene(name, NX, NY, *art.default_texture(name))
    quads = hs.quads()
    idx = np.arange(len(quads))
    assert len(idx) >= 1
    base = hs.nodes()
    results = [(art.refit_quads(hs.desc, quads, idx)[0], "library")]
    if len(quads) < 1000:                                             # (the restatement is a Python loop over the leaves)
        results.append((rq.refit(hs, idx, quads)[0], "restatement"))
    for got, who in results:
        assert np.array_equal(got["skip"], base["skip"]) and np.array_equal(got["prim"], base["prim"])
        rq.same_values(got["bmin"], base["bmin"], f"{name} {who} bmin")
        rq.same_values(got["bmax"], base["bmax"], f"{name} {who} bmax")
    prims = base["prim"][base["prim"] >= 0]
    if name == "cornell":
        assert ((prims >> 28) == sg.QUAD).sum() == 6 and hs.desc.n_boxes == 2
    if name == "crowd_big":
        assert len(prims) == 8401 and len(quads) == 15600
    hs.close()


def test_quad_record_and_box_records_are_the_host_librarys(art):
    """The binding's constructors give the records a flattened HostScene holds for the same arguments, and the restatement's."""
    matched = 0
    for name in ("quads", "cornell", "instanced", "fog"):
        hs = art.HostScene(name, NX, NY, *art.default_texture(name))
        quads, boxes = hs.quads(), rq.scene_boxes(hs)
        for k, q in enumerate(quads):
            made = art.quad_record(q["Q"], q["u"], q["v"], int(q["mat"]))
            assert made.tobytes() == rq.quad_record(q["Q"], q["u"], q["v"], int(q["mat"])).tobytes()
            if rq.is_inward(q):                                       # the reference's `inward` quads: the same record, facing the other way
                assert name == "cornell" and (made["n"] == -q["n"]).all() and made["D"] == -q["D"]
                assert rq.quad_record(q["Q"], q["u"], q["v"], int(q["mat"]), inward=True).tobytes() == quads[k:k + 1].tobytes()
                made["n"], made["D"] = q["n"], q["D"]
            else:
                matched += 1
            assert made.tobytes() == quads[k:k + 1].tobytes(), (name, k)
        for first in boxes:                                           # make_box's corners from its faces' origins: left, right, top, front
            faces = quads[first:first + 6]
            lo, hi = faces["Q"][3], np.array([faces["Q"][1][0], faces["Q"][4][1], faces["Q"][0][2]], np.float32)
            made = art.box_records(lo, hi, int(faces["mat"][0]))
            assert made.tobytes() == rq.box_records(lo, hi, int(faces["mat"][0])).tobytes()
            assert made.tobytes() == faces.tobytes(), (name, first)
            swapped = art.box_records(hi, lo, int(faces["mat"][0]))
            assert swapped.tobytes() == faces.tobytes()
            assert tuple(rq.axis_codes(made)) == rq.FACE_CODES
        hs.close()
    assert matched >= 40
    with pytest.raises(ValueError):
        art.quad_record((0, 0), (1, 0, 0), (0, 1, 0), 0)


def test_refusals_name_the_check_and_write_nothing(art):
    scene = _scene("general_plain", 0)
    L = art.rt_lib()
    quads = scene.quads()
    nodes_out, quads_out = np.full(len(scene.nodes()), 7, np.uint8).repeat(32), np.full(len(quads), 7, np.uint8).repeat(80)

    def refused(why, rec, idx=None, first=0, count=None, on=scene):
        u = art.RtQuadUpdate()
        rec = np.ascontiguousarray(rec)
        u.count, u.first = len(rec) if count is None else count, first
        u.quads = rec.ctypes.data if len(rec) else None
        keep = None if idx is None else np.ascontiguousarray(idx, np.int32)
        u.indices = None if keep is None else keep.ctypes.data
        assert L.rt_refit_quads(C.byref(on.desc), C.byref(u), nodes_out.ctypes.data, quads_out.ctypes.data) == 1
        assert L.rt_last_error_detail().decode() == why
        assert (nodes_out == 7).all() and (quads_out == 7).all()

    NON_FINITE, MATERIAL = "rt_refit_quads: a quad record has a non-finite Q, D, u, v, w or n", "rt_refit_quads: quad material out of range"
    RANGE, TWICE = "rt_refit_quads: quad index out of range", "rt_refit_quads: a quad index appears twice"
    MORE = "rt_refit_quads: more records than the scene has quads (an index is out of range or appears twice)"
    one = quads[3:4]
    assert L.rt_refit_quads(C.byref(scene.desc), None, nodes_out.ctypes.data, quads_out.ctypes.data) == 1
    assert L.rt_last_error_detail().decode() == "rt_refit_quads: null update"
    assert L.rt_refit_quads(None, None, None, None) == 1
    refused("rt_refit_quads: count is negative", one, count=-1)
    refused("rt_refit_quads: null quad records", quads[:0], count=1)
    refused(RANGE, one, idx=[len(quads)])
    refused(RANGE, one, idx=[-1])
    refused(RANGE, quads[:2], first=len(quads) - 1)
    refused(TWICE, quads[[0, 1, 0]], idx=[0, 1, 0])
    for field, value in (("Q", np.nan), ("D", np.inf), ("u", -np.inf), ("v", np.nan), ("w", np.inf), ("n", np.nan)):
        bad = one.copy()
        if field == "D":
            bad[field] = value
        else:
            bad[field][0, 1] = value
        refused(NON_FINITE, bad, idx=[3])
    # two faults at once, on four quads: a record is looked at as soon as its index has passed, the count before any index
    tiny = sg.tiny()
    few = tiny.quads()
    assert len(few) == 4
    bad = few[[0, 1]]
    bad["Q"][0, 1] = np.nan
    refused(NON_FINITE, bad, idx=[0, 4], on=tiny)                     # record 0 is bad, index 1 is out of range
    bad = few[[0, 1, 0]]
    bad["n"][1, 2] = np.nan
    refused(NON_FINITE, bad, idx=[0, 1, 0], on=tiny)                  # record 1 is bad, index 0 comes again as index 2
    refused(MORE, few[[0, 0, 1, 2, 3]], idx=[4, 0, 1, 2, 3], on=tiny) # too many records, index 0 is out of range
    for mat in (-1, scene.desc.n_materials):
        bad = one.copy()
        bad["mat"] = mat
        refused(MATERIAL, bad, idx=[3])
    with pytest.raises(ValueError, match="material"):
        art.refit_quads(scene.desc, bad, [3])
    with pytest.raises(ValueError, match="QUAD_DTYPE"):
        art.refit_quads(scene.desc, np.zeros((1, 20), np.float32))
    with pytest.raises(ValueError, match="one per record"):
        art.refit_quads(scene.desc, one, [0, 1])
    ok = one.copy()
    ok["pad0"], ok["pad1"], ok["pad2"] = np.nan, 5.0, -6.0            # pad0 is not looked at; pad1 and pad2 are kept
    _, out = art.refit_quads(scene.desc, ok, [3])
    assert out[3]["pad1"] == 5.0 and out[3]["pad2"] == -6.0
    # count == 0 is a successful no-op: the description comes back as it is
    nodes, out = art.refit_quads(scene.desc, quads[:0])
    assert nodes.tobytes() == scene.nodes().tobytes() and out.tobytes() == quads.tobytes()
    # a quad under an instance is allowed
    inst = scene.instances()
    under = int(inst["child"][(inst["child"] >> 28) == sg.QUAD][0]) & 0x0FFFFFFF
    art.refit_quads(scene.desc, quads[[under]], [under])


@pytest.mark.parametrize("recipe,seed,kind", [("general_plain", 0, "all"), ("general_plain", 4, "all"), ("general_plain", 0, "grow"),
                                               ("limits", 12, "one")])
def test_rule_boxes_contain_their_solids_by_the_oracle(art, orc, recipe, seed, kind):
    """A box that cut into its object would lose hits.  The oracle's frame of D' differs from the unmoved frame and equals, in
    every pixel and in its ray count, its frame of the same tree and records with every recomputed leaf boxed 12 units wider on
    every side -- more than the scene's extent, so that box holds the solid wherever a wrong rule could have put the rule's box."""
    scene = _scene(recipe, seed)
    idx, rec = rq.make_update(scene, kind)
    nodes, quads = art.refit_quads(scene.desc, rec, idx)
    moved = rq.Moved(scene, nodes, quads)
    first, _ = orc.OracleScene.from_host(scene, NX, NY).render(NS, seed_base=SEED)
    ruled, cnt = orc.OracleScene.from_host(moved, NX, NY).render(NS, seed_base=SEED)
    assert not np.array_equal(ruled, first)
    base = scene.nodes()
    leaf = np.flatnonzero(base["prim"] >= 0)
    flags = np.zeros(len(quads), bool)
    flags[idx] = True
    solids = rq.leaf_solids(base["prim"][leaf], scene.media())
    dep = np.array([rq.depends(s, flags, rq.scene_boxes(scene), scene.instances()) for s in solids])
    lo, hi = nodes["bmin"][leaf].copy(), nodes["bmax"][leaf].copy()
    lo[dep] -= np.float32(12.0)
    hi[dep] += np.float32(12.0)
    roomy = rq.Moved(scene, rq.refit_array(base, lo, hi), quads)
    outward, cnt2 = orc.OracleScene.from_host(roomy, NX, NY).render(NS, seed_base=SEED)
    differing = int((ruled.view(np.uint32) != outward.view(np.uint32)).any(-1).sum())
    assert differing == 0 and cnt["rays"] == cnt2["rays"], (differing, cnt["rays"], cnt2["rays"])
