"""What rt_reproject_quads must return ("temporal reprojection that follows moved quads and boxes", include/rt_abi.h): the
restatement of tests/reproject_expect.py called the way this entry is -- step 1 with the quad tail 1a''-1c'' in front of
rt_reproject_instances' 1a'-1c' and rt_reproject_moving's 1a-1c, step 2, step 3 with the carried normal and both id tests, step 4.
Ids and inst are required; the prim and the inst test of a tap are always on.

Here, shared by the host and the GPU tests: synthetic_quads(), the seeded buffers of the parity test with ids, inst planes and
tables that reach every branch of the three tails.
"""
from __future__ import annotations

import numpy as np

import reproject_expect as rx
import reproject_instances_expect as ix
import reproject_moving_expect as mx

F = np.float32
DEFAULTS = rx.DEFAULTS
QUAD_DTYPE, INSTANCE_DTYPE = rx.QUAD_DTYPE, rx.INSTANCE_DTYPE
ROTATE_Y, TRANSLATE = rx.ROTATE_Y, rx.TRANSLATE
SPHERE, QUAD, BOX, INSTANCE, MEDIUM = rx.SPHERE, rx.QUAD, rx.BOX, rx.INSTANCE, rx.MEDIUM
ref, dot, cross, followed_quad, quad_records_differ, planar = rx.ref, rx.dot, rx.cross, rx.followed_quad, rx.quad_records_differ, rx.planar
carry_point, carry_normal = rx.carry_on_quad, rx.normal_on_quad
to_object, to_world, rotate_in, rotate_out = rx.to_object, rx.to_world, rx.rotate_in, rx.rotate_out


def reproject(color, depth, alpha, cur, prev, **kw):
    """rx.reproject as rt_reproject_quads takes it: ids and inst are required, prev_inst exactly with a history."""
    assert kw.get("prim") is not None and kw.get("prev_prim") is not None and kw.get("inst") is not None, "ids and inst are required"
    assert (kw.get("prev_inst") is None) == (kw.get("history") is None)
    return rx.reproject(color, depth, alpha, cur, prev, **kw)


# ------------------------------------------------------------------------------------------- inputs of the parity test
def record(Q, u, v, mat=0):
    """One QUAD_DTYPE record (a 0-d array) of quad(Q, u, v): n, D and w as the constructor derives them, evaluated in double and
    rounded to float (the parity test needs records, not the host library's bits)."""
    r = np.zeros((), QUAD_DTYPE)
    Q, u, v = (np.asarray(x, np.float64) for x in (Q, u, v))
    nn = np.cross(u, v)
    with np.errstate(all="ignore"):
        unit = nn / np.sqrt(nn @ nn)
        r["Q"], r["u"], r["v"], r["mat"] = Q, u, v, mat
        r["n"], r["D"], r["w"] = unit, unit @ Q, nn / (nn @ nn)
    return r


# what each record of the quad tables is there for (index -> reason); quad_tables builds them in this order
QUAD_RECORDS = ["Q, u and v", "unmoved", "Q only", "u only", "v only", "n, w, D, mat and pads only: not moved", "nan Q", "infinite u",
                "zero w", "sheared and flipped"]
N_QUADS = len(QUAD_RECORDS)


def quad_tables():
    """(quads, prev_quads): the records of the parity test, near the points rx.synthetic's depths give."""
    cur = np.zeros(N_QUADS, QUAD_DTYPE)
    for k in range(N_QUADS):
        cur[k] = record((0.2 - 0.1 * k, -0.3 + 0.05 * k, 0.5 + 0.07 * k), (1.0 + 0.1 * k, 0.2, -0.1 * k), (0.1 * k, 0.9, 0.3 - 0.05 * k), mat=k)
    prev = cur.copy()
    prev[0] = record((0.35, -0.2, 0.4), (0.9, 0.3, 0.1), (-0.1, 1.2, 0.2), mat=0)
    prev["Q"][2] += np.array([0.05, -0.15, 0.1], F)
    prev["u"][3] += np.array([0.0, 0.25, 0.0], F)
    prev["v"][4] *= F(1.5)
    prev["n"][5], prev["w"][5], prev["D"][5], prev["mat"][5] = -cur["n"][5], cur["w"][5] * F(2), cur["D"][5] + F(1), 3
    prev["pad0"][5], prev["pad1"][5], prev["pad2"][5] = 1.0, 2.0, 3.0
    cur["Q"][6, 1] = np.nan
    prev["u"][7, 0] = np.inf
    cur["w"][8] = 0.0
    prev["Q"][8] += np.array([0.1, 0.1, 0.1], F)
    prev[9] = record(cur["Q"][9] + cur["u"][9], -cur["u"][9] + F(0.3) * cur["v"][9], cur["v"][9], mat=9)
    return cur, prev


def unmoved_quad_tables():
    """Tables of the same shape in which no record differs in Q, u or v (the NaN replaced: a NaN compares as moved); record 5 keeps
    its differences in the fields that do not enter the decision."""
    cur, prev = quad_tables()
    cur["Q"][6, 1] = 0.25
    same = cur.copy()
    for f in ("n", "w", "D", "mat", "pad0", "pad1", "pad2"):
        same[f][5] = prev[f][5]
    return cur, same


def id_palette():
    """ix.id_palette() and every quad of the tables, N_QUADS (the first out of range) and the largest index."""
    return np.concatenate([ix.id_palette(), np.array([ref(QUAD, k) for k in range(N_QUADS)] + [ref(QUAD, N_QUADS), ref(QUAD, 0x0FFFFFFF)], np.int32)])


def synthetic_quads(nx, ny, seed):
    """rx.synthetic's buffers with prim / prev_prim painted in 3 x 2 patches from id_palette() and inst / prev_inst in 4 x 3 patches
    from ix.inst_palette() -- the same patches in both frames, with one pixel in eight of each previous plane repainted at random,
    so that taps pass and fail both id tests -- and the tables of mx.tables(), ix.instance_tables() and quad_tables().  Half the
    prim patches show a quad of the tables; about a third of the frame shows no instance, a fifth the moved instance 0 and a fifth
    the unmoved instance 1, so that a moved quad meets each of them."""
    s = rx.synthetic(nx, ny, seed)
    rng = np.random.default_rng(seed + 3000)
    jj, ii = np.mgrid[0:ny, 0:nx]

    def paint(pal, weights, w, h):
        patch = (ii // w) + ((nx + w - 1) // w) * (jj // h)
        choice = rng.choice(len(pal), int(patch.max()) + 1, p=weights / weights.sum())
        if len(choice) >= len(pal):                      # every value at least once, wherever the frame has room for that
            choice[rng.permutation(len(choice))[:len(pal)]] = np.arange(len(pal))
        plane = pal[choice[patch]].astype(np.int32)
        before = plane.copy()
        again = rng.random((ny, nx)) < 0.125
        before[again] = pal[rng.integers(0, len(pal), int(again.sum()))]
        return plane, before

    pal = id_palette()
    weights = np.ones(len(pal))
    in_tables = (pal >= 0) & ((pal >> 28) == QUAD) & ((pal & 0x0FFFFFFF) < N_QUADS)
    weights[in_tables] = (len(pal) - in_tables.sum()) / in_tables.sum()
    prim, prev_prim = paint(pal, weights, 3, 2)
    ipal = ix.inst_palette()
    weights = np.ones(len(ipal))
    rest = len(ipal) - 3
    weights[0], weights[1], weights[2] = 1.25 * rest, 0.75 * rest, 0.75 * rest
    inst, prev_inst = paint(ipal, weights, 4, 3)
    b = dict(s["buffers"], prim=prim, prev_prim=prev_prim, inst=inst, prev_inst=prev_inst)
    spheres, prev_spheres, _, time, prev_time = mx.tables()
    instances, prev_instances, media = ix.instance_tables()
    quads, prev_quads = quad_tables()
    return {"cur": s["cur"], "cams": s["cams"], "buffers": b,
            "tables": dict(spheres=spheres, prev_spheres=prev_spheres, media=media, time=time, prev_time=prev_time, instances=instances,
                           prev_instances=prev_instances, quads=quads, prev_quads=prev_quads)}


select = ix.select


def without_quads(kw):
    """The same keyword arguments for reproject_instances_expect.reproject / rt_reproject_instances."""
    return {k: v for k, v in kw.items() if k not in ("quads", "prev_quads")}


# ------------------------------------------------------------------------------------ the real pairs of the GPU tests
def shows_moved(prim, inst, n_quads, n_instances, moved_indices):
    """Pixels whose step 1a'' quad is one of `moved_indices`."""
    return np.isin(followed_quad(prim, inst, n_quads, n_instances), np.asarray(moved_indices))


def box_extent(faces):
    """(a, b): per-axis min / max over the corners Q, Q + u, Q + v, (Q + u) + v of a box's six records, in float32."""
    corners = np.concatenate([faces["Q"], (faces["Q"] + faces["u"]).astype(F), (faces["Q"] + faces["v"]).astype(F),
                              ((faces["Q"] + faces["u"]).astype(F) + faces["v"]).astype(F)])
    return corners.min(axis=0), corners.max(axis=0)
