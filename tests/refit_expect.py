"""What rt_scene_update_spheres leaves behind, restated in NumPy float32 (include/rt_abi.h, "moving spheres"): the box rule, the
leaves that follow a sphere, the refit of a node array as unions over leaf ranges, and from them the description D' the update is
equivalent to, the tier arrays, the per-64-leaf unions and the scene's coordinate bound.  Shares no code with the library: the
interior boxes here are reductions over each node's range of leaves, the library's host statement walks child chains and its
kernels combine slots.

An update is (indices, records): int sphere indices and a SPHERE_DTYPE array.  Node arrays are NODE_DTYPE in the description's
encoding (skip = the next node's index); decode_device() brings a device read-back into it.
"""
import numpy as np

import accelerated_ray_tracer_amd as art
import scene_gen as sg

F32 = np.float32


def sphere_box(rec):
    """The box rule: r = |radius|, a = c0 + 0 vel, b = c0 + 1 vel, lo = min(a - r, b - r), hi = max(a + r, b + r); every
    operation on float32 arrays, so each is rounded once.  rec: SPHERE_DTYPE array (n,) -> lo, hi (n, 3)."""
    c0, vel = rec["c0"].astype(F32), rec["vel"].astype(F32)
    r = np.abs(rec["radius"].astype(F32))[..., None]
    a = c0 + F32(0.0) * vel
    b = c0 + F32(1.0) * vel
    return np.minimum(a - r, b - r), np.maximum(a + r, b + r)


def generator_box(rec):
    """scene_gen's own rule for a sphere leaf: float64 over the shutter [0, 1], rounded outward."""
    c0, v = rec["c0"].astype(np.float64), rec["vel"].astype(np.float64)
    rr = np.abs(rec["radius"].astype(np.float64))[..., None]
    return sg._down(np.minimum(c0, c0 + v) - rr), sg._up(np.maximum(c0, c0 + v) + rr)


def leaf_spheres(prims, media, n_spheres):
    """Per leaf prim: the sphere its box follows (its own, or its medium's direct boundary), else -1."""
    prims = np.asarray(prims, np.int64)
    out = np.full(len(prims), -1, np.int64)
    for q, p in enumerate(prims):
        if (p >> 28) == sg.MEDIUM:
            p = int(media["boundary"][p & 0x0FFFFFFF])
        if p >= 0 and (p >> 28) == sg.SPHERE and (p & 0x0FFFFFFF) < n_spheres:
            out[q] = p & 0x0FFFFFFF
    return out


def instanced(instances, n_spheres):
    under = np.zeros(n_spheres, bool)
    for c in instances["child"] if len(instances) else ():
        if c >= 0 and (c >> 28) == sg.SPHERE:
            under[c & 0x0FFFFFFF] = True
    return under


def direct_spheres(scene):
    """Indices of the spheres some leaf's box follows and no instance holds: the ones an update may move."""
    nodes, n_sph = scene.nodes(), len(scene.spheres())
    ls = leaf_spheres(nodes["prim"][nodes["prim"] >= 0], scene.media(), n_sph)
    ok = np.unique(ls[ls >= 0])
    return ok[~instanced(scene.instances(), n_sph)[ok]]


def decode_device(nodes):
    """A device node array (skip holds ~skip, an interior prim ~(index + 1)) in the description's encoding (interior prim -1)."""
    out = nodes.copy()
    out["skip"] = ~nodes["skip"]
    out["prim"] = np.where(nodes["prim"] < 0, -1, nodes["prim"])
    return out


def refit_array(nodes, leaf_lo, leaf_hi):
    """`nodes` with leaf q's box = (leaf_lo[q], leaf_hi[q]) and every interior box the min / max over the leaves of its subtree
    [i, skip[i]).  Links untouched."""
    out = nodes.copy()
    leaf = nodes["prim"] >= 0
    before = np.concatenate([[0], np.cumsum(leaf)])
    assert before[-1] == len(leaf_lo)
    for i in range(len(nodes)):
        a, b = int(before[i]), int(before[int(nodes["skip"][i])])
        if leaf[i]:
            assert b == a + 1
        if b > a:
            out["bmin"][i] = leaf_lo[a:b].min(0)
            out["bmax"][i] = leaf_hi[a:b].max(0)
    return out


def refit(scene, indices, records, rule=sphere_box, nodes=None):
    """D' of `scene` (anything with HostScene's surface) under the update: (nodes, spheres, leaf_lo, leaf_hi).  nodes: another
    array over the same leaves (a decoded walk array) to refit instead of the description's."""
    base = scene.nodes()
    spheres = scene.spheres()
    indices = np.asarray(indices, np.int64)
    spheres[indices] = records
    moved = np.zeros(len(spheres), bool)
    moved[indices] = True
    leaf = base["prim"] >= 0
    lo, hi = base["bmin"][leaf].astype(F32), base["bmax"][leaf].astype(F32)
    ls = leaf_spheres(base["prim"][leaf], scene.media(), len(spheres))
    follow = (ls >= 0) & moved[np.maximum(ls, 0)]
    if follow.any():
        lo[follow], hi[follow] = rule(spheres[ls[follow]])
    tree = base if nodes is None else nodes
    assert np.array_equal(tree["prim"][tree["prim"] >= 0], base["prim"][leaf])
    return refit_array(tree, lo, hi), spheres, lo, hi


def slot_ranges(lo, hi):
    """Per 64 leaves the union of their boxes: (slots, 8) = lo, hi, 0, 0."""
    slots = (len(lo) + 63) // 64
    out = np.zeros((slots, 8), F32)
    for k in range(slots):
        out[k, 0:3] = lo[k * 64:(k + 1) * 64].min(0)
        out[k, 3:6] = hi[k * 64:(k + 1) * 64].max(0)
    return out


def bound(lo, hi):
    if len(lo) == 0:
        return np.zeros(3, F32)
    return np.maximum(np.abs(lo), np.abs(hi)).max(0).astype(F32)


UPDATES = ["one", "all", "moving", "negative", "far"]


def make_update(scene, kind):
    """(indices, records) of the named update of `scene`; deterministic."""
    direct = direct_spheres(scene)
    assert len(direct) > 0
    sph = scene.spheres()
    rng = np.random.default_rng(len(direct) * 7 + UPDATES.index(kind))
    pick = direct[[len(direct) // 2]]
    if kind == "all":
        idx = direct[rng.permutation(len(direct))]                   # out of order, as an index list may be
        rec = sph[idx]
        rec["c0"] += rng.uniform(-0.4, 0.4, (len(idx), 3)).astype(np.float32)
        return idx, rec
    rec = sph[pick]
    if kind == "one":
        rec["c0"] += np.array([0.3, 0.2, -0.25], np.float32)
    elif kind == "moving":
        rec["vel"] = np.array([0.2, 0.5, -0.1], np.float32)
    elif kind == "negative":
        rec["radius"] = -0.9 * np.abs(rec["radius"])
    elif kind == "far":
        rec["c0"] += np.array([500.0, 0.0, -600.0], np.float32)
    return pick, rec


class Moved:
    """Anything with HostScene's surface with other node and sphere arrays in its description (D'); every other array is the
    original's, which is kept alive here."""

    def __init__(self, scene, nodes, spheres, name="/moved"):
        self.original = scene
        self._nodes, self._spheres = np.ascontiguousarray(nodes, art.NODE_DTYPE), np.ascontiguousarray(spheres, art.SPHERE_DTYPE)
        assert len(self._nodes) == scene.desc.n_nodes and len(self._spheres) == scene.desc.n_spheres
        self.name = getattr(scene, "name", "desc") + name
        self.desc = art.RtSceneDesc.from_buffer_copy(scene.desc)
        self.desc.nodes = self._nodes.ctypes.data if len(self._nodes) else None
        self.desc.spheres = self._spheres.ctypes.data if len(self._spheres) else None
        self.nx, self.ny, self.ns, self.gamma = scene.nx, scene.ny, scene.ns, scene.gamma
        self.background, self.use_gradient_bg = scene.background, scene.use_gradient_bg
        for k in ("materials", "media", "instances", "quads"):
            setattr(self, k, getattr(scene, k))
        self.frame = lambda **kw: art.HostScene.frame(self, **kw)

    def nodes(self): return self._nodes.copy()
    def spheres(self): return self._spheres.copy()

    def close(self):
        pass


def moved_scene(scene, indices, records, rule=sphere_box):
    nodes, spheres, _, _ = refit(scene, indices, records, rule)
    return Moved(scene, nodes, spheres)


def same_values(got, want, what):
    """Equal as floats (so +0 == -0), with no NaN on either side."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any() and not np.isnan(want).any(), what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
