"""What rt_reproject_instances must return ("temporal reprojection that follows moved instances", include/rt_abi.h): the
restatement of tests/reproject_expect.py called the way this entry is -- step 1 with the instance tail 1a'-1c' in front of
rt_reproject_moving's 1a-1c, step 2, step 3 with the carried normal and the inst test, step 4.  Ids and inst are required; the prim
and the inst test of a tap are always on.

Here, shared by the host and the GPU tests: synthetic_instances(), the seeded buffers of the parity test with ids, inst planes
and tables that reach every branch of both tails.
"""
from __future__ import annotations

import numpy as np

import reproject_expect as rx
import reproject_moving_expect as mx

F = np.float32
DEFAULTS = rx.DEFAULTS
INSTANCE_DTYPE = rx.INSTANCE_DTYPE
ROTATE_Y, TRANSLATE = rx.ROTATE_Y, rx.TRANSLATE
SPHERE, QUAD, BOX, INSTANCE, MEDIUM = rx.SPHERE, rx.QUAD, rx.BOX, rx.INSTANCE, rx.MEDIUM
ref, followed_instance, records_differ = rx.ref, rx.followed_instance, rx.records_differ
carry_point, carry_normal = rx.carry_on_instance, rx.turn_with_instance


def reproject(color, depth, alpha, cur, prev, **kw):
    """rx.reproject as rt_reproject_instances takes it: ids and inst are required, prev_inst exactly with a history, and no quad
    table is passed.  details: every entry of rx.reproject's; "followed" are the pixels that took step 1c'."""
    assert kw.get("prim") is not None and kw.get("prev_prim") is not None and kw.get("inst") is not None, "ids and inst are required"
    assert (kw.get("prev_inst") is None) == (kw.get("history") is None)
    assert "quads" not in kw and "prev_quads" not in kw
    return rx.reproject(color, depth, alpha, cur, prev, **kw)


# ------------------------------------------------------------------------------------------- inputs of the parity test
def record(angle_degrees=None, offset=None, child=0):
    """One INSTANCE_DTYPE record (a 0-d array) of translate(rotate_y(child, angle), offset), either half left out when None; sin and
    cos in double, rounded to float."""
    r = np.zeros((), INSTANCE_DTYPE)
    r["cos_t"] = 1.0
    r["child"] = child
    if angle_degrees is not None:
        r["sin_t"], r["cos_t"], r["flags"] = np.sin(np.radians(angle_degrees)), np.cos(np.radians(angle_degrees)), ROTATE_Y
    if offset is not None:
        r["offset"], r["flags"] = offset, r["flags"] | TRANSLATE
    return r


# what each record of the instance tables is there for (index -> reason); instance_tables builds them in this order
INSTANCE_RECORDS = ["angle and offset", "unmoved", "offset only", "angle only", "flags only: rotate gained", "flags only: translate lost",
                    "flags 0, another offset", "flags 7", "nan sin_t", "infinite previous offset", "no sine / cosine pair", "bounds a medium"]
N_INSTANCES = len(INSTANCE_RECORDS)
N_MEDIA = 9


def instance_tables():
    """(instances, prev_instances, media): the records of the parity test, and mx.tables()' media extended by boundaries that are
    instances in and out of range."""
    cur = np.zeros(N_INSTANCES, INSTANCE_DTYPE)
    for k in range(N_INSTANCES):
        cur[k] = record(3.0 + 2.0 * k, (0.05 * k, -0.02 * k, 0.1 - 0.03 * k), child=ref(BOX, k))
    prev = cur.copy()
    prev[0] = record(-2.0, (0.12, 0.05, -0.08), child=ref(BOX, 0))
    prev["offset"][2] += np.array([0.15, -0.1, 0.05], F)
    prev[3] = record(1.5, cur["offset"][3], child=ref(BOX, 3))
    prev["flags"][4] = TRANSLATE                                     # the current frame gained the rotation
    cur["flags"][5] = ROTATE_Y                                       # ... and lost the translation
    cur["flags"][6] = prev["flags"][6] = 0                           # moved by the rule, carried by nothing
    prev["offset"][6] += np.array([0.3, 0.0, 0.0], F)
    cur["flags"][7] = prev["flags"][7] = 7                           # a bit outside 1..3 is only ever tested
    prev["sin_t"][7], prev["cos_t"][7] = np.sin(np.radians(14.0)), np.cos(np.radians(14.0))
    cur["sin_t"][8] = np.nan
    prev["offset"][9, 1] = np.inf
    cur["sin_t"][10], cur["cos_t"][10] = 0.8, 0.9
    prev["sin_t"][10], prev["cos_t"][10] = 0.5, 0.5
    prev[11] = record(20.0, (0.6, -0.1, -0.2), child=ref(SPHERE, 0))
    cur["child"][11] = ref(SPHERE, 0)
    media = np.zeros(N_MEDIA, mx.MEDIUM_DTYPE)
    media["boundary"] = list(mx.tables()[2]["boundary"]) + [ref(INSTANCE, 11), ref(INSTANCE, N_INSTANCES), ref(INSTANCE, 0x0FFFFFFF)]
    media["neg_inv_density"] = -1.0
    assert ref(INSTANCE, 0) == media["boundary"][5]
    return cur, prev, media


def unmoved_instance_tables():
    """Tables of the same shape in which no record differs (the NaN replaced: a NaN compares as moved)."""
    cur, _, media = instance_tables()
    cur["sin_t"][8] = 0.3
    return cur, cur.copy(), media


def id_palette():
    """mx.id_palette() for N_MEDIA media: media 6..8 are in range here, N_MEDIA is the first that is not."""
    return np.concatenate([mx.id_palette(), np.array([ref(MEDIUM, 7), ref(MEDIUM, 8), ref(MEDIUM, N_MEDIA)], np.int32)])


def inst_palette():
    """The values the inst planes are painted with: none (-1), every record, out of range, and negative but not -1."""
    return np.array([-1] + list(range(N_INSTANCES)) + [N_INSTANCES, 0x7FFFFFFF, -2, -2147483648], np.int32)


def synthetic_instances(nx, ny, seed):
    """rx.synthetic's buffers with prim / prev_prim painted in 3 x 2 patches from id_palette() and inst / prev_inst in 4 x 3 patches
    from inst_palette() -- the same patches in both frames, with one pixel in eight of each previous plane repainted at random,
    so that taps pass and fail both id tests -- and the tables of mx.tables() and instance_tables().  About half the frame shows
    no instance; the media come up more often than the other ids, so that every boundary rule decides pixels."""
    s = rx.synthetic(nx, ny, seed)
    rng = np.random.default_rng(seed + 2000)
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
    weights[[1, 10]] = 3.0
    weights[(pal >= 0) & ((pal >> 28) == MEDIUM)] = 3.0
    prim, prev_prim = paint(pal, weights, 3, 2)
    ipal = inst_palette()
    weights = np.ones(len(ipal))
    weights[0] = len(ipal)
    inst, prev_inst = paint(ipal, weights, 4, 3)
    b = dict(s["buffers"], prim=prim, prev_prim=prev_prim, inst=inst, prev_inst=prev_inst)
    spheres, prev_spheres, _, time, prev_time = mx.tables()
    instances, prev_instances, media = instance_tables()
    return {"cur": s["cur"], "cams": s["cams"], "buffers": b,
            "tables": dict(spheres=spheres, prev_spheres=prev_spheres, media=media, time=time, prev_time=prev_time, instances=instances,
                           prev_instances=prev_instances)}


def select(buffers, normals, history=True):
    """The keyword arguments of reproject() with the normal test on or off; ids and inst always."""
    keep = ["color", "depth", "alpha", "prim", "prev_prim", "inst"] + (["history", "history_len", "prev_depth", "prev_alpha", "prev_inst"] if history else [])
    keep += ["normal", "prev_normal"] if normals else []
    return {k: buffers[k] for k in keep}


def without_inst(kw):
    """The same keyword arguments for reproject_moving_expect.reproject / rt_reproject_moving."""
    return {k: v for k, v in kw.items() if k not in ("inst", "prev_inst", "instances", "prev_instances")}


# ------------------------------------------------------------------------------------ the real pairs of the GPU tests
def turned(records, indices, degrees, shift=(0.0, 0.0, 0.0)):
    """The records `indices` of an INSTANCE_DTYPE array turned by `degrees` more (angles through atan2 in double, sin and cos rounded
    to float) and, where they translate, shifted by `shift`."""
    rec = records[np.asarray(indices)].copy()
    for k in range(len(rec)):
        d = degrees[k] if np.ndim(degrees) else degrees
        a = np.arctan2(float(rec["sin_t"][k]), float(rec["cos_t"][k])) + np.radians(d)
        rec["sin_t"][k], rec["cos_t"][k] = np.sin(a), np.cos(a)
        rec["flags"][k] |= ROTATE_Y
        if rec["flags"][k] & TRANSLATE:
            rec["offset"][k] += np.asarray(shift, F)
    return rec


def shows_moved(inst, prim, media, n_instances, moved_indices):
    """Pixels whose step 1a' instance is one of `moved_indices`."""
    return np.isin(followed_instance(inst, prim, n_instances, media), np.asarray(moved_indices))
