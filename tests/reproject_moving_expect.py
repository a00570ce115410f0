"""What rt_reproject_moving must return ("temporal reprojection that follows moved spheres", include/rt_abi.h): the restatement of
tests/reproject_expect.py called the way this entry is -- step 1 with its tail 1a-1c, then steps 2-4.  Ids are required and the id
test of a tap is always on.

Here, shared by the host and the GPU tests: synthetic_moving(), the seeded buffers of the parity test with ids and tables
that reach every branch of the tail, so that the properties which keep the test from testing nothing are checked on the very
inputs the GPU test uses.
"""
from __future__ import annotations

import numpy as np

import reproject_expect as rx

F = np.float32
DEFAULTS = rx.DEFAULTS
SPHERE_DTYPE, MEDIUM_DTYPE = rx.SPHERE_DTYPE, rx.MEDIUM_DTYPE
SPHERE, QUAD, BOX, INSTANCE, MEDIUM = rx.SPHERE, rx.QUAD, rx.BOX, rx.INSTANCE, rx.MEDIUM
ref, shutter_centre, followed_sphere = rx.ref, rx.shutter_centre, rx.followed_sphere


def reproject(color, depth, alpha, cur, prev, details=None, **kw):
    """rx.reproject as rt_reproject_moving takes it: ids are required, and nothing of the instance and quad forms is passed.
    details: a dict that receives "followed" (ny, nx), the pixels that took step 1c, and "sphere", the result of step 1a."""
    assert not set(kw) & {"inst", "prev_inst", "instances", "prev_instances", "quads", "prev_quads"}
    assert kw.get("prim") is not None and kw.get("prev_prim") is not None, "ids are required"
    d = {}
    result = rx.reproject(color, depth, alpha, cur, prev, details=d, **kw)
    if details is not None:
        details["followed"], details["sphere"] = d["followed_sphere"], d["sphere"]
    return result


# ------------------------------------------------------------------------------------------- inputs of the parity test
N_SPHERES = 10
# what each record of the tables is there for (index -> reason); synthetic_moving builds them in this order
RECORDS = ["moved", "unmoved", "radius only", "previous radius 0", "current radius 0", "negative radius", "nan c0", "infinite vel",
           "velocity, time != prev_time", "moved further"]


def tables():
    """(spheres, prev_spheres, media, time, prev_time) of the parity test."""
    cur = np.zeros(N_SPHERES, SPHERE_DTYPE)
    cur["c0"] = np.array([0.1, -0.2, 0.4], F) + np.arange(N_SPHERES, dtype=F)[:, None] * np.array([0.05, 0.02, -0.03], F)
    cur["radius"] = 1.0
    cur["mat"] = np.arange(N_SPHERES)
    prev = cur.copy()
    prev["c0"][0] += np.array([0.06, -0.04, 0.02], F)                         # moved
    prev["radius"][2] = 0.9                                                    # radius only
    prev["radius"][3] = 0.0                                                    # previous radius 0: everything lands on the centre
    cur["radius"][4] = 0.0                                                     # current radius 0: a division by zero
    cur["radius"][5], prev["radius"][5] = -1.0, -1.25                          # negative radius (a flipped sphere)
    prev["c0"][5] += np.array([0.0, 0.03, 0.0], F)
    cur["c0"][6, 1] = np.nan                                                   # NaN compares as moved
    cur["vel"][7, 0] = np.inf                                                  # an infinite centre in the current frame only
    cur["vel"][8] = prev["vel"][8] = np.array([0.2, -0.1, 0.05], F)           # the same record in both frames, followed by time alone
    prev["c0"][9] += np.array([-0.3, 0.2, 0.1], F)
    prev["radius"][9] = 1.1
    media = np.zeros(6, MEDIUM_DTYPE)
    media["boundary"] = [ref(SPHERE, 0), ref(QUAD, 1), -1, ref(SPHERE, N_SPHERES), ref(SPHERE, 0x0FFFFFFF), ref(INSTANCE, 0)]
    media["neg_inv_density"] = -1.0
    return cur, prev, media, F(0.5), F(0.25)


def unmoved_tables():
    """Tables of the same shape in which no record moved: both frames hold the current records (the NaN replaced: a NaN compares
    as moved) at one instant."""
    cur, _, media, time, _ = tables()
    cur["c0"][6, 1] = 0.25
    return cur, cur.copy(), media, time, time


def id_palette():
    """The ids the synthetic frames are painted with: every branch of step 1a."""
    n_media = 6
    return np.array([-1, ref(SPHERE, 0), ref(SPHERE, 1), ref(SPHERE, 2), ref(SPHERE, 3), ref(SPHERE, 4), ref(SPHERE, 5), ref(SPHERE, 6),
                     ref(SPHERE, 7), ref(SPHERE, 8), ref(SPHERE, 9), ref(SPHERE, N_SPHERES), ref(SPHERE, 0x0FFFFFFF), ref(QUAD, 0), ref(QUAD, 3),
                     ref(MEDIUM, 0), ref(MEDIUM, 1), ref(MEDIUM, 2), ref(MEDIUM, 3), ref(MEDIUM, 4), ref(MEDIUM, 5), ref(MEDIUM, n_media),
                     ref(MEDIUM, 0x0FFFFFFF), ref(BOX, 2), ref(5, 3), ref(7, 0x0FFFFFFF), -2147483648, -2], np.int32)


def synthetic_moving(nx, ny, seed):
    """rx.synthetic's buffers with prim / prev_prim painted over in small patches from id_palette() -- the same patches in both
    frames, with one pixel in eight of the previous frame repainted at random, so that taps pass and fail the id test -- and the
    tables of tables().  The moved sphere and the medium it bounds come up more often than the rest."""
    s = rx.synthetic(nx, ny, seed)
    rng = np.random.default_rng(seed + 1000)
    pal = id_palette()
    weights = np.ones(len(pal))
    weights[[1, 10, 15]] = 4.0
    jj, ii = np.mgrid[0:ny, 0:nx]
    patch = (ii // 3) + ((nx + 2) // 3) * (jj // 2)
    choice = rng.choice(len(pal), int(patch.max()) + 1, p=weights / weights.sum())
    if len(choice) >= len(pal):                      # every id at least once, wherever the frame has room for that
        choice[rng.permutation(len(choice))[:len(pal)]] = np.arange(len(pal))
    prim = pal[choice[patch]].astype(np.int32)
    prev_prim = prim.copy()
    again = rng.random((ny, nx)) < 0.125
    prev_prim[again] = pal[rng.integers(0, len(pal), int(again.sum()))]
    b = dict(s["buffers"], prim=prim, prev_prim=prev_prim)
    spheres, prev_spheres, media, time, prev_time = tables()
    return {"cur": s["cur"], "cams": s["cams"], "buffers": b,
            "tables": dict(spheres=spheres, prev_spheres=prev_spheres, media=media, time=time, prev_time=prev_time)}


def select(buffers, normals, history=True):
    """The keyword arguments of reproject() with the normal test on or off; ids always."""
    keep = ["color", "depth", "alpha", "prim", "prev_prim"] + (["history", "history_len", "prev_depth", "prev_alpha"] if history else [])
    keep += ["normal", "prev_normal"] if normals else []
    return {k: buffers[k] for k in keep}


# -------------------------------------------------------------------------------------- the real pair of the GPU test
# general_tex's direct spheres that the 64 x 48 frame shows, and what happens to them between the two frames
REAL_MOVE = np.array([0.0, 0.35, 0.0], F)
REAL_GROW = F(1.15)


def real_update(scene, count=6):
    """(indices, records): the `count` largest direct spheres of `scene` that are not its ground, lifted by REAL_MOVE, every other
    one also grown by REAL_GROW."""
    import refit_expect as rf
    sph = scene.spheres()
    direct = rf.direct_spheres(scene)
    direct = direct[np.abs(sph["radius"][direct]) < 100.0]
    idx = direct[np.argsort(-np.abs(sph["radius"][direct]), kind="stable")[:count]]
    rec = sph[idx]
    rec["c0"] += REAL_MOVE
    rec["radius"][::2] *= REAL_GROW
    return idx.astype(np.int32), rec
