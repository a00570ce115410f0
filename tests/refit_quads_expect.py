"""What rt_scene_update_quads leaves behind, restated in NumPy float32 (include/rt_abi.h, "moving quads and boxes"): the axis code
and the canonical-box mark the device derives from quad records, the solid a leaf's box follows and when it depends on an
updated quad, and from them the description D' the update is equivalent to; a quad constructor in binary32 operation order.
Shares no code with the library; the box rules are tests/refit_instances_expect.py's, the interior boxes, slot unions and the
bound tests/refit_expect.py's reductions over leaf ranges.

An update is (indices, records): int quad indices and a QUAD_DTYPE array.
"""
import numpy as np

import accelerated_ray_tracer_amd as art
import refit_expect as rf
import refit_instances_expect as ri
import scene_gen as sg
from refit_expect import bound, decode_device, refit_array, same_values, slot_ranges  # noqa: F401  (shared with the tests)
from refit_instances_expect import scene_boxes, scene_spheres

F32 = np.float32
FACE_CODES = (3, 1, 3, 1, 2, 2)                  # a canonical box: normals along z, x, z, x, y, y, as codes 1 + axis
CANONICAL, FIRST_MASK = 0x40000000, 0x3FFFFFFF


# ---------------------------------------------------------------------------------------------------- derived device data
def axis_code(q):
    """1 + C when the quad's unit normal is exactly +-e_C, w lies on C alone and is non-zero, u and v have no C component and
    each exactly one non-zero component, on different axes; else 0.  q: one QUAD_DTYPE record."""
    n, w, u, v = (np.asarray(q[k], F32) for k in ("n", "w", "u", "v"))
    for c in range(3):
        a, b = (c + 1) % 3, (c + 2) % 3
        if not (abs(float(n[c])) == 1.0 and n[a] == 0 and n[b] == 0):
            continue
        if not (w[a] == 0 and w[b] == 0 and w[c] != 0 and u[c] == 0 and v[c] == 0):
            continue
        on = lambda x: {k for k in (a, b) if x[k] != 0}   # noqa: E731
        if len(on(u)) == 1 and len(on(v)) == 1 and on(u) != on(v):
            return 1 + c
    return 0


def axis_codes(quads):
    return np.array([axis_code(q) for q in quads], np.int32)


def device_records(quads, boxes):
    """What rt_scene_create keeps of a description's quads and boxes (rt_debug_scene_quads): pad0 = the axis code as integer bits,
    bit 30 of first_quad set for a box whose six faces carry FACE_CODES in order.  Decided per box: ranges may overlap."""
    codes = axis_codes(quads)
    out = quads.copy()
    out["pad0"] = codes.view(F32)
    words = np.asarray(boxes, np.int32).copy()
    for k, first in enumerate(words):
        if tuple(codes[first:first + 6]) == FACE_CODES:
            words[k] = first | CANONICAL
    return out, words


# ---------------------------------------------------------------------------------------------------- leaves
def leaf_solids(prims, media):
    """Per leaf prim: its solid -- the primitive, or its medium's boundary -- as a prim ref."""
    out = np.asarray(prims, np.int64).copy()
    for q, p in enumerate(out):
        if (p >> 28) == sg.MEDIUM:
            out[q] = int(media["boundary"][p & 0x0FFFFFFF])
    return out


def depends(solid, moved, boxes, instances):
    """Whether a solid depends on a quad marked in `moved`: a quad itself, a box by any of its six faces, an instance by its child."""
    kind, i = int(solid) >> 28, int(solid) & 0x0FFFFFFF
    if kind == sg.INSTANCE:
        return depends(int(instances["child"][i]), moved, boxes, instances)
    if kind == sg.QUAD:
        return bool(moved[i])
    if kind == sg.BOX:
        first = int(boxes[i]) & FIRST_MASK
        return bool(moved[first:first + 6].any())
    return False


def solid_box(solid, spheres, quads, boxes, instances):
    kind, i = int(solid) >> 28, int(solid) & 0x0FFFFFFF
    if kind == sg.INSTANCE:
        rec = instances[i]
        return ri.instance_box(rec, *ri.child_box(rec["child"], spheres, quads, boxes))
    return ri.child_box(solid, spheres, quads, boxes)


def refit(scene, indices, records, nodes=None):
    """D' of `scene` under the update: (nodes, quads, leaf_lo, leaf_hi).  nodes: another array over the same leaves (a decoded
    walk array) to refit instead of the description's."""
    base = scene.nodes()
    quads = scene.quads()
    indices = np.asarray(indices, np.int64)
    quads[indices] = records
    moved = np.zeros(len(quads), bool)
    moved[indices] = True
    leaf = base["prim"] >= 0
    lo, hi = base["bmin"][leaf].astype(F32), base["bmax"][leaf].astype(F32)
    solids = leaf_solids(base["prim"][leaf], scene.media())
    spheres, boxes, inst = scene_spheres(scene), scene_boxes(scene), scene.instances()
    for q, s in enumerate(solids):
        if depends(s, moved, boxes, inst):
            lo[q], hi[q] = solid_box(s, spheres, quads, boxes, inst)
    tree = base if nodes is None else nodes
    assert np.array_equal(tree["prim"][tree["prim"] >= 0], base["prim"][leaf])
    return refit_array(tree, lo, hi), quads, lo, hi


class Moved(ri.Moved):
    """D' as a scene: the original with other node and quad (and, for the mixed tests, instance and sphere) arrays."""

    def __init__(self, scene, nodes, quads, instances=None, spheres=None, name="/requadded"):
        super().__init__(scene, nodes, scene.instances() if instances is None else instances, spheres, name)
        self._quads = np.ascontiguousarray(quads, art.QUAD_DTYPE)
        assert len(self._quads) == scene.desc.n_quads
        self.desc.quads = self._quads.ctypes.data if len(self._quads) else None
        self.quads = lambda: self._quads.copy()


def moved_scene(scene, indices, records):
    nodes, quads, _, _ = refit(scene, indices, records)
    return Moved(scene, nodes, quads)


# ---------------------------------------------------------------------------------------------------- constructors
def fma32(a, x, b):
    """fmaf on scalars, rounded once (refit_instances_expect.fma32 gives an array of one)."""
    return F32(ri.fma32(a, x, b).reshape(-1)[0])


def _dot(a, b):
    """vec3.cuh's dot as the reference's compiler contracts it: fma(a2, b2, fma(a0, b0, a1 b1))."""
    return fma32(a[2], b[2], fma32(a[0], b[0], F32(a[1]) * F32(b[1])))


def quad_record(Q, u, v, mat, inward=False):
    """quad::quad (the reference's quad.cuh:29-54) in binary32 operation order: n = cross(u, v) with one fma per component,
    normal = n / |n| (negated when inward), D = dot(normal, Q), w = n / dot(n, n).  One QUAD_DTYPE record, shape (1,)."""
    Q, u, v = (np.asarray(x, F32).reshape(3) for x in (Q, u, v))
    n = np.array([fma32(u[1], v[2], -(u[2] * v[1])), -fma32(u[0], v[2], -(u[2] * v[0])), fma32(u[0], v[1], -(u[1] * v[0]))], F32)
    normal = (n / np.sqrt(_dot(n, n))).astype(F32)
    if inward:
        normal = -normal
    rec = np.zeros(1, art.QUAD_DTYPE)
    rec["Q"], rec["u"], rec["v"], rec["mat"] = Q, u, v, mat
    rec["n"], rec["D"], rec["w"] = normal, _dot(normal, Q), (n / _dot(n, n)).astype(F32)
    return rec


def box_records(a, b, mat):
    """make_box (quad.cuh:145-162): front, right, back, left, top, bottom.  Six QUAD_DTYPE records."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    z = F32(0)
    ex, ey, ez = np.array([hi[0] - lo[0], z, z], F32), np.array([z, hi[1] - lo[1], z], F32), np.array([z, z, hi[2] - lo[2]], F32)
    faces = [((lo[0], lo[1], hi[2]), ex, ey), ((hi[0], lo[1], hi[2]), -ez, ey), ((hi[0], lo[1], lo[2]), -ex, ey),
             ((lo[0], lo[1], lo[2]), ez, ey), ((lo[0], hi[1], hi[2]), ex, -ez), ((lo[0], lo[1], lo[2]), ex, ez)]
    return np.concatenate([quad_record(Q, u, v, mat) for Q, u, v in faces])


def is_inward(rec):
    """Whether a record's normal is the negated constructor normal (the reference's `inward` quads, scene_gen's `flip`)."""
    made = quad_record(rec["Q"], rec["u"], rec["v"], 0)
    return bool(np.dot(made["n"][0].astype(np.float64), np.asarray(rec["n"], np.float64)) < 0)


def reshaped(rec, Q, u, v):
    """The record `rec` (one element) with another Q, u, v: material, facing and pads kept, D, w, n made anew."""
    new = quad_record(Q, u, v, int(rec["mat"]), is_inward(rec))
    new["pad1"], new["pad2"] = rec["pad1"], rec["pad2"]
    return new[0]


def shifted(rec, d):
    return reshaped(rec, np.asarray(rec["Q"], F32) + np.asarray(d, F32), rec["u"], rec["v"])


# ---------------------------------------------------------------------------------------------------- the scene's quads, sorted
def census(scene):
    """Which quads and boxes the leaves reach and how: direct quads (a leaf's own primitive), direct boxes, boxes under an
    instance, every box's face indices, the codes of all quads."""
    nodes, quads, boxes, inst = scene.nodes(), scene.quads(), scene_boxes(scene), scene.instances()
    prims = nodes["prim"][nodes["prim"] >= 0].astype(np.int64)
    direct_quads = [int(p & 0x0FFFFFFF) for p in prims if (p >> 28) == sg.QUAD]
    direct_boxes = [int(p & 0x0FFFFFFF) for p in prims if (p >> 28) == sg.BOX]
    solids = leaf_solids(prims, scene.media())
    inst_boxes = []
    for s in solids:
        if (int(s) >> 28) == sg.INSTANCE:
            c = int(inst["child"][int(s) & 0x0FFFFFFF])
            if (c >> 28) == sg.BOX and (c & 0x0FFFFFFF) not in inst_boxes:
                inst_boxes.append(c & 0x0FFFFFFF)
    codes = axis_codes(quads)
    canonical = [k for k, f in enumerate(boxes) if tuple(codes[f:f + 6]) == FACE_CODES]
    return dict(direct_quads=direct_quads, direct_boxes=direct_boxes, inst_boxes=inst_boxes, codes=codes, canonical=canonical,
                boxes=boxes, quads=quads)


def _size(rec):
    return F32(max(np.abs(rec["u"]).max(), np.abs(rec["v"]).max()))


UPDATES = ["one", "all", "tilt", "shear", "grow", "identity"]


def kinds_for(scene):
    """The update kinds `scene` has the objects for."""
    c = census(scene)
    out = ["all", "identity"]
    if c["direct_quads"]:
        out += ["one", "tilt"]
    if c["canonical"]:
        out.append("shear")
    if c["inst_boxes"]:
        out.append("grow")
    return [k for k in UPDATES if k in out]


def make_update(scene, kind):
    """(indices, records) of the named update of `scene`; deterministic.  The move back is (indices, scene.quads()[indices]);
    for `shear` that is the second update, which must bring bit 30 back."""
    c = census(scene)
    quads, boxes, codes = c["quads"], c["boxes"], c["codes"]
    rng = np.random.default_rng(len(quads) * 13 + UPDATES.index(kind))
    if kind == "identity":
        idx = np.arange(len(quads))
        return idx, quads[idx]
    if kind == "all":                    # every quad, out of order; the faces of one box move together, so that it stays closed
        step = rng.uniform(-0.15, 0.15, (len(quads), 3)).astype(F32)
        for first in boxes:
            step[first:first + 6] = step[first] * F32(0.5)
        idx = rng.permutation(len(quads))
        rec = quads[idx]
        for k, i in enumerate(idx):
            rec[k] = shifted(quads[i], step[i] * _size(quads[i]))
        return idx, rec
    if kind == "one":                    # a direct quad, translated and resized
        i = c["direct_quads"][len(c["direct_quads"]) // 2]
        q, s = quads[i], _size(quads[i])
        rec = quads[[i]]
        rec[0] = reshaped(q, q["Q"] + s * np.array([0.3, 0.2, -0.25], F32), q["u"] * F32(1.25), q["v"] * F32(0.75))
        return np.array([i]), rec
    if kind == "tilt":                   # an axis-aligned direct quad becomes oblique (code 1..3 -> 0), an oblique one aligned (0 -> 1..3)
        aligned = [i for i in c["direct_quads"] if codes[i] != 0]
        oblique = [i for i in c["direct_quads"] if codes[i] == 0]
        idx, rec = [], []
        if aligned:
            i = aligned[len(aligned) // 2]
            q, axis = quads[i], int(codes[i]) - 1
            u = q["u"].copy()
            u[axis] = F32(0.35) * _size(q)
            idx.append(i)
            rec.append(reshaped(q, q["Q"], u, q["v"]))
            assert axis_code(rec[-1]) == 0
        if oblique:
            i = max(oblique, key=lambda k: float(quads[k]["Q"][2]))      # the one nearest the generated scenes' camera
            q = quads[i]
            lu, lv = F32(np.linalg.norm(q["u"])), F32(np.linalg.norm(q["v"]))
            idx.append(i)
            rec.append(reshaped(q, q["Q"], np.array([lu, 0, 0], F32), np.array([0, lv, 0], F32)))
            assert axis_code(rec[-1]) == 3
        assert idx
        return np.array(idx), np.array(rec, art.QUAD_DTYPE)
    if kind == "shear":                  # the top face of a canonical box leans: bit 30 must drop (a direct box if there is one)
        pick = [b for b in c["canonical"] if b in c["direct_boxes"]] or c["canonical"]
        first = int(boxes[pick[len(pick) // 2]])
        i = first + 4
        q = quads[i]
        v = q["v"].copy()
        v[1] = F32(0.4) * _size(q)
        rec = quads[[i]]
        rec[0] = reshaped(q, q["Q"], q["u"], v)
        assert axis_code(rec[0]) == 0 and codes[i] == 2
        return np.array([i]), rec
    assert kind == "grow"                # the six faces of a box under an instance: make_box of another size, the faces' materials kept
    first = int(boxes[c["inst_boxes"][0]])
    faces = quads[first:first + 6]
    corners = np.concatenate([faces["Q"], faces["Q"] + faces["u"], faces["Q"] + faces["v"]])
    lo, hi = corners.min(0), corners.max(0)
    rec = box_records(lo, lo + (hi - lo) * np.array([1.3, 1.6, 0.7], F32), 0)
    rec["mat"], rec["pad1"], rec["pad2"] = faces["mat"], faces["pad1"], faces["pad2"]
    return np.arange(first, first + 6), rec
