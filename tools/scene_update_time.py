#!/usr/bin/env python3
"""Wall time of rt_scene_update_spheres per call -- one moved sphere, and every direct sphere moved, from host records and from a
device tensor -- beside the wall time of rt_scene_create of the same scene (tools/scene_create_time.py's method: the call alone,
the best of a few, the first reported apart); and of rt_scene_update_instances -- one instance, and every instance -- beside
rt_scene_update_spheres and rt_scene_create on scenes with instances; and of rt_scene_update_quads -- one quad,
and every quad -- beside rt_scene_update_instances and rt_scene_create of the same scenes.  One JSON line per
measurement.

    python tools/scene_update_time.py                       # this tree: creation and updates
    python tools/scene_update_time.py --only instances      # the scenes with instances alone
    python tools/scene_update_time.py --only quads          # the scenes of the quad update alone
    python tools/scene_update_time.py --create-only --root DIR --label parent
                                                            # creation alone, with the package of another checkout (the parent
                                                            # commit, built in DIR), for the comparison DESIGN.md 4.15 quotes
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package is imported")
ap.add_argument("--create-only", action="store_true")
ap.add_argument("--label", default="this tree")
ap.add_argument("--calls", type=int, default=40, help="timed update calls per measurement (the median is reported)")
ap.add_argument("--only", choices=("spheres", "instances", "quads"), default=None, help="one of the three scene lists")
ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np  # noqa: E402
import accelerated_ray_tracer_amd as art  # noqa: E402

# the random scene (488 spheres), Book-2 final (1008 spheres, every one direct in this flattening: the cluster's rotation and
# translation are baked into its centres) and a 4096-leaf scene
SCENES = (("random_scene", 1200, 800), ("final", 800, 800), ("crowd_4096", 64, 64))
# the Cornell box (two rotated blocks), every instance kind (18 instances, 128 leaves) and 1 200 rotated boxes among 8 401 leaves
INSTANCE_SCENES = (("cornell", 600, 600), ("instanced", 64, 64), ("crowd_big", 64, 64))
# the Cornell box (18 quads: six direct ones, two boxes under instances), a generated scene with every way a leaf reaches a quad
# (tests/scene_gen.py, general_plain seed 0: 58 quads, 45 leaves) and 15 600 quads among 8 401 leaves
QUAD_SCENES = (("cornell", 600, 600), ("general_plain/0", 48, 32), ("crowd_big", 64, 64))


def emit(**rec):
    line = json.dumps(dict(rec, label=args.label))
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def direct_spheres(hs):
    """The spheres some leaf's box follows -- a leaf's own sphere, or the direct boundary of a leaf's medium -- that no instance holds."""
    nodes, media, inst, n = hs.nodes(), hs.media(), hs.instances(), hs.desc.n_spheres
    prim = nodes["prim"][nodes["prim"] >= 0].astype(np.int64)
    is_medium = (prim >> 28) == art.RT_PRIM_MEDIUM
    if is_medium.any():
        prim[is_medium] = media["boundary"][prim[is_medium] & 0x0FFFFFFF]
    direct = np.unique(prim[(prim >= 0) & ((prim >> 28) == art.RT_PRIM_SPHERE)] & 0x0FFFFFFF)
    child = inst["child"].astype(np.int64) if len(inst) else np.zeros(0, np.int64)
    under = np.unique(child[(child >= 0) & ((child >> 28) == art.RT_PRIM_SPHERE)] & 0x0FFFFFFF)
    return np.setdiff1d(direct[direct < n], under).astype(np.int32)


def time_create(hs, scene):
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        ds = art.DeviceScene(hs)
        ts.append((time.perf_counter() - t0) * 1e3)
        info = ds.walk_info()
        ds.close()
    emit(what="rt_scene_create", scene=scene, ms_min=round(min(ts), 3), ms_first=round(ts[0], 3), spheres=hs.desc.n_spheres,
         nodes_reference=info["nodes_reference"], nodes_walked=info["nodes_walked"])


def time_updates(hs, scene, ds=None):
    import torch
    L = art.rt_lib()
    keep = ds is not None
    ds = ds or art.DeviceScene(hs)
    direct = direct_spheres(hs)
    if len(direct) == 0:
        emit(what="rt_scene_update_spheres", scene=scene, note="no direct sphere")
        return
    sph = hs.spheres()
    rng = np.random.default_rng(1)

    def call(u, on_device):
        t0 = time.perf_counter()
        st = L.rt_scene_update_spheres(ds._p, C.byref(u), on_device, 0, None)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0, L.rt_last_error_detail().decode()
        return dt

    first_call = None
    for size, idx in (("one", direct[len(direct) // 2:len(direct) // 2 + 1]), ("all", direct)):
        for source in ("host", "device"):
            ts = []
            for k in range(5 + args.calls):                                      # five warm-up calls, then the timed ones
                rec = sph[idx]
                rec["c0"] += rng.uniform(-0.2, 0.2, (len(idx), 3)).astype(np.float32)
                u = art.RtSphereUpdate()
                u.count, u.indices = len(idx), idx.ctypes.data
                if source == "device":
                    t = torch.from_numpy(rec.view(np.float32).reshape(-1, 8).copy()).cuda()
                    torch.cuda.synchronize()
                    u.spheres = t.data_ptr()
                else:
                    u.spheres = rec.ctypes.data
                dt = call(u, 1 if source == "device" else 0)
                if first_call is None:
                    first_call = dt                                              # builds the scene's lookup tables
                elif k >= 5:
                    ts.append(dt)
            emit(what="rt_scene_update_spheres", scene=scene, moved=size, records=source, count=int(len(idx)), calls=len(ts),
                 ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
    emit(what="rt_scene_update_spheres, first call of the scene (builds the lookup tables)", scene=scene, ms=round(first_call, 3))
    f = hs.frame(nx=min(hs.nx, 240), ny=min(hs.ny, 160), ns=4)
    _, st = ds.render(f)                                                         # the moved scene still renders
    assert st.rays > 0
    if not keep:
        ds.close()


def time_instance_updates(hs, scene):
    """rt_scene_update_instances: one instance and every instance, a new offset and (for the rotated ones) a new angle per call."""
    import torch
    L = art.rt_lib()
    ds = art.DeviceScene(hs)
    inst = hs.instances()
    every = np.arange(len(inst), dtype=np.int32)
    rng = np.random.default_rng(2)
    first_call = None
    for size, idx in (("one", every[len(every) // 2:len(every) // 2 + 1]), ("all", every)):
        for source in ("host", "device"):
            ts = []
            for k in range(5 + args.calls):
                rec = inst[idx]
                a = np.arctan2(rec["sin_t"].astype(np.float64), rec["cos_t"].astype(np.float64)) + rng.uniform(-0.3, 0.3, len(idx))
                rot = (rec["flags"] & art.RT_INST_ROTATE_Y) != 0
                rec["sin_t"][rot], rec["cos_t"][rot] = np.sin(a)[rot], np.cos(a)[rot]
                tr = (rec["flags"] & art.RT_INST_TRANSLATE) != 0
                rec["offset"][tr] += rng.uniform(-0.2, 0.2, (int(tr.sum()), 3)).astype(np.float32)
                u = art.RtInstanceUpdate()
                u.count, u.indices = len(idx), idx.ctypes.data
                if source == "device":
                    t = torch.from_numpy(rec.view(np.float32).reshape(-1, 8).copy()).cuda()
                    torch.cuda.synchronize()
                    u.instances = t.data_ptr()
                else:
                    u.instances = rec.ctypes.data
                t0 = time.perf_counter()
                st = L.rt_scene_update_instances(ds._p, C.byref(u), 1 if source == "device" else 0, 0, None)
                dt = (time.perf_counter() - t0) * 1e3
                assert st == 0, L.rt_last_error_detail().decode()
                if first_call is None:
                    first_call = dt                                              # builds the scene's lookup tables
                elif k >= 5:
                    ts.append(dt)
            emit(what="rt_scene_update_instances", scene=scene, moved=size, records=source, count=int(len(idx)), calls=len(ts),
                 ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
    emit(what="rt_scene_update_instances, first call of the scene (builds the lookup tables)", scene=scene, ms=round(first_call, 3))
    time_updates(hs, scene, ds)                                                  # the sphere update of the same scene, same tables
    ds.close()


def time_quad_updates(hs, scene):
    """rt_scene_update_quads: one quad and every quad, displaced anew per call (Q moves, D = n . Q follows)."""
    import torch
    L = art.rt_lib()
    ds = art.DeviceScene(hs)
    quads = hs.quads()
    every = np.arange(len(quads), dtype=np.int32)
    size = np.maximum(np.abs(quads["u"]).max(1), np.abs(quads["v"]).max(1))
    rng = np.random.default_rng(3)
    first_call = None
    for moved, idx in (("one", every[len(every) // 2:len(every) // 2 + 1]), ("all", every)):
        for source in ("host", "device"):
            ts = []
            for k in range(5 + args.calls):
                rec = quads[idx]
                rec["Q"] += (rng.uniform(-0.05, 0.05, (len(idx), 3)) * size[idx, None]).astype(np.float32)
                rec["D"] = (rec["n"].astype(np.float64) * rec["Q"]).sum(1)
                u = art.RtQuadUpdate()
                u.count, u.indices = len(idx), idx.ctypes.data
                if source == "device":
                    t = torch.from_numpy(rec.view(np.float32).reshape(-1, 20).copy()).cuda()
                    torch.cuda.synchronize()
                    u.quads = t.data_ptr()
                else:
                    u.quads = rec.ctypes.data
                t0 = time.perf_counter()
                st = L.rt_scene_update_quads(ds._p, C.byref(u), 1 if source == "device" else 0, 0, None)
                dt = (time.perf_counter() - t0) * 1e3
                assert st == 0, L.rt_last_error_detail().decode()
                if first_call is None:
                    first_call = dt                                              # builds the scene's lookup tables
                elif k >= 5:
                    ts.append(dt)
            emit(what="rt_scene_update_quads", scene=scene, moved=moved, records=source, count=int(len(idx)), calls=len(ts),
                 ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
    emit(what="rt_scene_update_quads, first call of the scene (builds the lookup tables)", scene=scene, ms=round(first_call, 3))
    f = hs.frame(nx=min(hs.nx, 240), ny=min(hs.ny, 160), ns=4)
    _, st = ds.render(f)                                                         # the changed scene still renders
    assert st.rays > 0
    ds.close()


def quad_scene(scene, nx, ny):
    if "/" not in scene:
        img, iw, ih = art.default_texture(scene)
        return art.HostScene(scene, nx, ny, img, iw, ih)
    sys.path.insert(0, os.path.join(os.path.abspath(args.root), "tests"))
    import scene_gen
    recipe, seed = scene.split("/")
    return scene_gen.generate(recipe, int(seed), nx, ny)


if not args.create_only:
    import torch
    if not torch.cuda.is_available():                                            # (before rt_init, as the test suite does)
        raise SystemExit("no GPU visible to torch: the device-tensor measurements need one")
art.init(0)
for scene, nx, ny in SCENES if args.only in (None, "spheres") else ():
    img, iw, ih = art.default_texture(scene)
    hs = art.HostScene(scene, nx, ny, img, iw, ih)
    time_create(hs, scene)
    if not args.create_only:
        time_updates(hs, scene)
    hs.close()
for scene, nx, ny in INSTANCE_SCENES if args.only in (None, "instances") else ():
    img, iw, ih = art.default_texture(scene)
    hs = art.HostScene(scene, nx, ny, img, iw, ih)
    time_create(hs, scene)
    if not args.create_only:
        time_instance_updates(hs, scene)
    hs.close()
for scene, nx, ny in QUAD_SCENES if args.only in (None, "quads") else ():
    hs = quad_scene(scene, nx, ny)
    time_create(hs, scene)
    if not args.create_only:
        time_quad_updates(hs, scene)
        time_instance_updates(hs, scene)                                         # the instance (and sphere) updates of the same scene
    hs.close()
