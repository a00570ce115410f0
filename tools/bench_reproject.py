#!/usr/bin/env python3
"""rt_reproject and rt_scene_set_camera on an MI355X.

(a) rt_reproject at 1200 x 800 with every guide on (normals, ids, motion) and with none: the headline scene under two cameras
    3 degrees apart, its 4-spp frames and feature buffers on the device.  Median of 20 calls between device events (device
    tensors, nothing allocated or copied inside the window).  Yardsticks from the same process: one unstaged iteration of
    rt_denoise at the same size (option denoise_lds = 0; the total at K = 2 minus the total at K = 1, i.e. without the pack
    pass) -- 25 taps where this kernel has 4 -- and a device-to-device copy of the bytes a pixel of rt_reproject must move at
    the least with every guide on (36 B of the current frame + 24 B written: a copy of 30 B per pixel reads 30 and writes 30).
(b) What a stale cost prior costs: rt_render of the headline scene at 1200 x 800, 500 spp, after a 20 degree set_camera with
    recalibrate 0 and with 1, against a scene created for that camera.  The three alternate, medians of `--frames` frames of
    stats.ms_render each; set_camera's own host time (with and without recalibration) and rt_scene_create's beside them.
--kernel-loop N instead enqueues N calls of rt_reproject with every guide, N with none and N of rt_denoise (K = 3, unstaged)
and exits: the run to put under `rocprofv3 --kernel-trace --stats`, whose per-kernel averages are the device times -- between
events a single call of either is dominated by the host side of the call (argument and pointer checks, the launch).
--kernel-stats FILE reads that run's kernel_stats.csv and prints / appends the rows of the two kernels as one JSON line.
--moving-loop N --moved {none,all} is the moving mode (rt_reproject_moving, profiles/reproject_moving_mi355x.jsonl): the headline
scene at 1200 x 800 under the two cameras, the second frame rendered after every small sphere (radius < 0.5) was lifted by
update_spheres; N times rt_reproject with every guide and rt_reproject_moving with every guide, alternating, on those same
buffers -- with `none` the tables hold the second frame's records twice (no sphere moved: every pixel takes the static path
after the records were read), with `all` the records of both frames.  It exits after the loop: the run to put under
`rocprofv3 --kernel-trace --stats`; --kernel-stats FILE --moved X then appends the two kernels' rows and their ratio.
--instances-loop N --moved {none,all} [--scene NAME] is the instance mode (rt_reproject_instances,
profiles/reproject_instances_mi355x.jsonl): an instanced scene (default cornell) at 1200 x 800 under its own camera and one 3
degrees further round, the second frame rendered after every rotated instance was turned by 6 degrees through update_instances; N
times rt_reproject_moving (no sphere table, the scene's media) and rt_reproject_instances with every guide, alternating, on those
same buffers -- with `none` the tables hold the second frame's records twice (every instance pixel takes the static path after the
records were read), with `all` the records of both frames.  It exits after the loop; --kernel-stats FILE --moved X --instances
then appends the two kernels' rows and their ratio.
--quads-loop N --moved {none,all} [--scene NAME] is the quad mode (rt_reproject_quads, profiles/reproject_quads_mi355x.jsonl): a
scene with boxes (default cornell) at 1200 x 800 under its own camera and one 3 degrees further round, the second frame rendered
after every box was made a fifth taller through update_quads; N times rt_reproject_instances (no sphere table, the scene's media,
the scene's unmoved instance records) and rt_reproject_quads with every guide, alternating, on those same buffers -- with `none`
the quad tables hold the second frame's records twice, with `all` the records of both frames.  It exits after the loop;
--kernel-stats FILE --moved X --quads then appends the two kernels' rows and their ratio.
--orbit-pair N is the stale prior in an animation loop: ONE scene, its camera switched between the 0 and the 20 degree view
(recalibrate 0) before every frame, 2 N + 2 frames, the first two left out.  Since the cost map a scene that
renders one view again runs warm, one-part frames, so (b)'s three scenes no longer show what a stale prior costs; here every
frame's prior is the other view's -- the stale map, or, with a library from before the map, the stale calibration frame.
One JSON line per measurement goes to stdout and, with --out, is appended to that file (profiles/reproject_mi355x.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accelerated_ray_tracer_amd as art  # noqa: E402

EYE, LOOKAT = (13.0, 2.0, 3.0), (0.0, 0.0, 0.0)      # host/rtw_scenes.cpp, bouncing_spheres


def orbited(degrees, nx, ny):
    th = np.radians(degrees)
    eye = (np.cos(th) * EYE[0] + np.sin(th) * EYE[2], EYE[1], -np.sin(th) * EYE[0] + np.cos(th) * EYE[2])
    return art.make_camera(eye, LOOKAT, (0, 1, 0), 30.0, nx / ny, 0.1, float(np.linalg.norm(EYE)), 0.0, 1.0)


def median_ms(fn, calls=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def moving_loop(args, hs, dev):
    """The moving mode: see the module's text."""
    nx, ny = args.nx, args.ny
    ds = art.DeviceScene(hs)
    f4 = hs.frame(nx=nx, ny=ny, ns=4, gamma=1.0)
    cams = [orbited(0.0, nx, ny), orbited(3.0, nx, ny)]
    before = ds.spheres()
    small = (before["radius"] > 0) & (before["radius"] < 0.5)
    after = before.copy()
    after["c0"][small, 1] += np.float32(0.3)
    host = []
    for k, cam in enumerate(cams):
        if k:
            ds.update_spheres(after)
        ds.set_camera(cam)
        color, _ = ds.render(f4)
        host.append(dict(ds.render_aov(f4, ids=True), color=color))
    t = [{k: torch.from_numpy(v).to(dev) for k, v in h.items()} for h in host]
    words = lambda rec: torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(len(rec), -1).copy()).to(dev)   # noqa: E731
    cur_records, prev_records = words(after), words(before if args.moved == "all" else after)
    media = words(hs.media()) if len(hs.media()) else None
    first = art.reproject(t[0]["color"], t[0]["depth"], t[0]["alpha"], cams[0], cams[0])
    out, out_len = torch.empty_like(first.out), torch.empty_like(first.length)
    motion = torch.empty((ny, nx, 2), dtype=torch.float32, device=dev)
    kw = dict(history=first.out, history_len=first.length, prev_depth=t[0]["depth"], prev_alpha=t[0]["alpha"], out=out, out_len=out_len,
              stream=torch.cuda.current_stream(dev).cuda_stream, blocking=False, normal=t[1]["normal"], prim=t[1]["prim"],
              prev_normal=t[0]["normal"], prev_prim=t[0]["prim"], motion=motion)
    on_small = np.isin(host[1]["prim"], np.flatnonzero(small)) & (host[1]["alpha"] >= 0.5)
    for _ in range(args.moving_loop):
        art.reproject(t[1]["color"], t[1]["depth"], t[1]["alpha"], cams[1], cams[0], **kw)
        static_found = float((out_len > 1).float().mean().item())
        art.reproject(t[1]["color"], t[1]["depth"], t[1]["alpha"], cams[1], cams[0], spheres=cur_records, prev_spheres=prev_records, media=media, **kw)
        moving_found = float((out_len > 1).float().mean().item())
    torch.cuda.synchronize()
    print(json.dumps({"what": "rt_reproject_moving loop", "spheres_moved": args.moved, "calls_each": args.moving_loop, "spheres": int(len(before)),
                      "small_spheres": int(small.sum()), "pixels_on_small_spheres": round(float(on_small.mean()), 4),
                      "pixels_with_history_static": round(static_found, 4), "pixels_with_history_moving": round(moving_found, 4)}))
    ds.close()


CORNELL_EYE, CORNELL_LOOKAT = (278.0, 278.0, -800.0), (278.0, 278.0, 0.0)      # host/rtw_scenes.cpp, cornell_camera


def instances_loop(args, dev):
    """The instance mode: see the module's text."""
    nx, ny = args.nx, args.ny
    hs = art.HostScene(args.scene, nx, ny)
    ds = art.DeviceScene(hs)
    f4 = hs.frame(nx=nx, ny=ny, ns=4, gamma=1.0)
    built = art.RtCamera.from_buffer_copy(hs.desc.camera)
    if args.scene.startswith("cornell"):
        th = np.radians(3.0)
        d = np.subtract(CORNELL_EYE, CORNELL_LOOKAT)
        eye = np.add(CORNELL_LOOKAT, (np.cos(th) * d[0] + np.sin(th) * d[2], d[1], -np.sin(th) * d[0] + np.cos(th) * d[2]))
        cams = [built, art.make_camera(eye, CORNELL_LOOKAT, (0, 1, 0), 40.0, nx / ny, 0.0, 800.0, 0.0, 1.0)]
    else:
        cams = [built, built]
    before = ds.instances()
    rotated = (before["flags"] & art.RT_INST_ROTATE_Y) != 0
    after = before.copy()
    a = np.arctan2(before["sin_t"].astype(np.float64), before["cos_t"].astype(np.float64)) + np.radians(6.0)
    after["sin_t"][rotated], after["cos_t"][rotated] = np.sin(a)[rotated], np.cos(a)[rotated]
    host = []
    for k, cam in enumerate(cams):
        if k:
            ds.update_instances(after)
        ds.set_camera(cam)
        color, _ = ds.render(f4)
        host.append(dict(ds.render_aov(f4, ids=True), color=color))
    t = [{k: torch.from_numpy(v).to(dev) for k, v in h.items()} for h in host]
    words = lambda rec: torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(len(rec), -1).copy()).to(dev)   # noqa: E731
    cur_records, prev_records = words(after), words(before if args.moved == "all" else after)
    media = words(hs.media()) if len(hs.media()) else None
    no_spheres = torch.empty((0, 8), dtype=torch.int32, device=dev)
    first = art.reproject(t[0]["color"], t[0]["depth"], t[0]["alpha"], cams[0], cams[0])
    out, out_len = torch.empty_like(first.out), torch.empty_like(first.length)
    motion = torch.empty((ny, nx, 2), dtype=torch.float32, device=dev)
    kw = dict(history=first.out, history_len=first.length, prev_depth=t[0]["depth"], prev_alpha=t[0]["alpha"], out=out, out_len=out_len,
              stream=torch.cuda.current_stream(dev).cuda_stream, blocking=False, normal=t[1]["normal"], prim=t[1]["prim"],
              prev_normal=t[0]["normal"], prev_prim=t[0]["prim"], motion=motion, media=media)
    on_rotated = np.isin(host[1]["inst"], np.flatnonzero(rotated)) & (host[1]["alpha"] >= 0.5)
    sel = torch.from_numpy(on_rotated).to(dev)
    for _ in range(args.instances_loop):
        art.reproject(t[1]["color"], t[1]["depth"], t[1]["alpha"], cams[1], cams[0], spheres=no_spheres, prev_spheres=no_spheres, **kw)
        moving_found, moving_on = float((out_len > 1).float().mean().item()), float((out_len[sel] > 1).float().mean().item())
        art.reproject(t[1]["color"], t[1]["depth"], t[1]["alpha"], cams[1], cams[0], instances=cur_records, prev_instances=prev_records,
                      inst=t[1]["inst"], prev_inst=t[0]["inst"], **kw)
        inst_found, inst_on = float((out_len > 1).float().mean().item()), float((out_len[sel] > 1).float().mean().item())
    torch.cuda.synchronize()
    print(json.dumps({"what": "rt_reproject_instances loop", "scene": args.scene, "instances_moved": args.moved, "calls_each": args.instances_loop,
                      "instances": int(len(before)), "rotated_instances": int(rotated.sum()), "pixels_on_rotated_instances": round(float(on_rotated.mean()), 4),
                      "pixels_with_history_moving": round(moving_found, 4), "pixels_with_history_instances": round(inst_found, 4),
                      "of_rotated_instance_pixels_moving": round(moving_on, 4), "of_rotated_instance_pixels_instances": round(inst_on, 4)}))
    ds.close()
    hs.close()


def box_firsts(quads):
    """The first quad of every six consecutive records that are the faces of one axis-aligned box in make_box's order."""
    axis = [int(np.flatnonzero(q["n"])[0]) if np.count_nonzero(q["n"]) == 1 else -1 for q in quads]
    return [f for f in range(len(quads) - 5) if axis[f:f + 6] == [2, 0, 2, 0, 1, 1] and len(set(quads["mat"][f:f + 6].tolist())) == 1]


def grown_boxes(quads, factor):
    """`quads` with every box rebuilt by the host library's make_box at `factor` times its height (rayTracer --grow's rule)."""
    rec = quads.copy()
    for f in box_firsts(quads):
        six = quads[f:f + 6]
        corners = np.concatenate([six["Q"], six["Q"] + six["u"], six["Q"] + six["v"], (six["Q"] + six["u"]) + six["v"]])
        a, b = corners.min(axis=0), corners.max(axis=0)
        b[1] = np.float32(float(a[1]) + (float(b[1]) - float(a[1])) * factor)
        rec[f:f + 6] = art.box_records(a, b, int(six["mat"][0]))
    return rec


def quads_loop(args, dev):
    """The quad mode: see the module's text."""
    nx, ny = args.nx, args.ny
    hs = art.HostScene(args.scene, nx, ny)
    ds = art.DeviceScene(hs)
    f4 = hs.frame(nx=nx, ny=ny, ns=4, gamma=1.0)
    built = art.RtCamera.from_buffer_copy(hs.desc.camera)
    if args.scene.startswith("cornell"):
        th = np.radians(3.0)
        d = np.subtract(CORNELL_EYE, CORNELL_LOOKAT)
        eye = np.add(CORNELL_LOOKAT, (np.cos(th) * d[0] + np.sin(th) * d[2], d[1], -np.sin(th) * d[0] + np.cos(th) * d[2]))
        cams = [built, art.make_camera(eye, CORNELL_LOOKAT, (0, 1, 0), 40.0, nx / ny, 0.0, 800.0, 0.0, 1.0)]
    else:
        cams = [built, built]
    before = ds.quads()
    after = grown_boxes(before, 1.2)
    faces = [q for f in box_firsts(before) for q in range(f, f + 6)]
    host = []
    for k, cam in enumerate(cams):
        if k:
            ds.update_quads(after)
            after = ds.quads()
        ds.set_camera(cam)
        color, _ = ds.render(f4)
        host.append(dict(ds.render_aov(f4, ids=True), color=color))
    t = [{k: torch.from_numpy(v).to(dev) for k, v in h.items()} for h in host]
    words = lambda rec: torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(len(rec), -1).copy()).to(dev)   # noqa: E731
    cur_records, prev_records = words(after), words(before if args.moved == "all" else after)
    instances = words(ds.instances())
    media = words(hs.media()) if len(hs.media()) else None
    first = art.reproject(t[0]["color"], t[0]["depth"], t[0]["alpha"], cams[0], cams[0])
    out, out_len = torch.empty_like(first.out), torch.empty_like(first.length)
    motion = torch.empty((ny, nx, 2), dtype=torch.float32, device=dev)
    kw = dict(history=first.out, history_len=first.length, prev_depth=t[0]["depth"], prev_alpha=t[0]["alpha"], out=out, out_len=out_len,
              stream=torch.cuda.current_stream(dev).cuda_stream, blocking=False, normal=t[1]["normal"], prim=t[1]["prim"],
              prev_normal=t[0]["normal"], prev_prim=t[0]["prim"], motion=motion, media=media, instances=instances, prev_instances=instances,
              inst=t[1]["inst"], prev_inst=t[0]["inst"])
    prim = host[1]["prim"].astype(np.int64)
    on_faces = (prim >= 0) & ((prim >> 28) == art.RT_PRIM_QUAD) & np.isin(prim & 0x0FFFFFFF, faces) & (host[1]["alpha"] >= 0.5)
    sel = torch.from_numpy(on_faces).to(dev)
    for _ in range(args.quads_loop):
        art.reproject(t[1]["color"], t[1]["depth"], t[1]["alpha"], cams[1], cams[0], **kw)
        inst_found, inst_on = float((out_len > 1).float().mean().item()), float((out_len[sel] > 1).float().mean().item())
        art.reproject(t[1]["color"], t[1]["depth"], t[1]["alpha"], cams[1], cams[0], quads=cur_records, prev_quads=prev_records, **kw)
        quad_found, quad_on = float((out_len > 1).float().mean().item()), float((out_len[sel] > 1).float().mean().item())
    torch.cuda.synchronize()
    print(json.dumps({"what": "rt_reproject_quads loop", "scene": args.scene, "quads_moved": args.moved, "calls_each": args.quads_loop,
                      "quads": int(len(before)), "box_faces": len(faces), "pixels_on_box_faces": round(float(on_faces.mean()), 4),
                      "pixels_with_history_instances": round(inst_found, 4), "pixels_with_history_quads": round(quad_found, 4),
                      "of_box_face_pixels_instances": round(inst_on, 4), "of_box_face_pixels_quads": round(quad_on, 4)}))
    ds.close()
    hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=800)
    ap.add_argument("--ns", type=int, default=500)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-loop", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--moving-loop", type=int, default=0)
    ap.add_argument("--moved", choices=["none", "all"], default=None)
    ap.add_argument("--orbit-pair", type=int, default=0)
    ap.add_argument("--instances-loop", type=int, default=0)
    ap.add_argument("--instances", action="store_true", help="with --kernel-stats: the instance mode's two kernels")
    ap.add_argument("--quads-loop", type=int, default=0)
    ap.add_argument("--quads", action="store_true", help="with --kernel-stats: the quad mode's two kernels")
    ap.add_argument("--scene", default="cornell")
    args = ap.parse_args()
    nx, ny = args.nx, args.ny
    if args.kernel_stats:
        import csv
        rows = {}
        with open(args.kernel_stats) as fh:
            for r in csv.DictReader(fh):
                name = r["Name"]
                if "rt_reproject_kernel" in name or "rt_denoise_kernel" in name or "rt_denoise_pack_kernel" in name:
                    rows[name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")] = {
                        "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3), "min_us": round(float(r["MinNs"]) / 1e3, 3),
                        "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
        line = {"what": "device time per kernel (rocprofv3 --kernel-trace --stats)", "nx": nx, "ny": ny, "kernels": rows}
        if args.moved and args.quads:
            instances = rows.get("rt_reproject_kernel<true, true, true, rt_reproject_follow_instance_params>")
            following = rows.get("rt_reproject_kernel<true, true, true, rt_reproject_follow_quad_params>")
            line["quads_moved"], line["scene"] = args.moved, args.scene
            if instances and following:
                line["quads_over_instances"] = round(following["average_us"] / instances["average_us"], 4)
        elif args.moved and args.instances:
            moving = rows.get("rt_reproject_kernel<true, true, true, rt_reproject_follow_params>")
            following = rows.get("rt_reproject_kernel<true, true, true, rt_reproject_follow_instance_params>")
            line["instances_moved"], line["scene"] = args.moved, args.scene
            if moving and following:
                line["instances_over_moving"] = round(following["average_us"] / moving["average_us"], 4)
        elif args.moved:
            static = rows.get("rt_reproject_kernel<true, true, true>")
            moving = rows.get("rt_reproject_kernel<true, true, true, rt_reproject_follow_params>")
            line["spheres_moved"] = args.moved
            if static and moving:
                line["moving_over_static"] = round(moving["average_us"] / static["average_us"], 4)
        print(json.dumps(line))
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
        return
    art.init(0)
    dev = torch.device("cuda", 0)
    if args.instances_loop:
        instances_loop(args, dev)
        return
    if args.quads_loop:
        quads_loop(args, dev)
        return
    hs = art.HostScene("random_scene", nx, ny)
    lines = []

    if args.moving_loop:
        moving_loop(args, hs, dev)
        return

    if args.orbit_pair:
        ds = art.DeviceScene(hs)
        cams = [orbited(0.0, nx, ny), orbited(20.0, nx, ny)]
        f = hs.frame(nx=nx, ny=ny, ns=args.ns)
        fb = torch.empty((ny, nx, 3), dtype=torch.float32, device=dev)
        ms = []
        for it in range(2 * args.orbit_pair + 2):
            ds.set_camera(cams[it & 1])
            _, st = ds.render(f, out=fb.data_ptr())
            if it >= 2:
                ms.append(st.ms_render)
        line = {"what": "rt_render, the camera switched between two views 20 degrees apart before every frame, recalibrate 0", "scene": "random_scene",
                "nx": nx, "ny": ny, "ns": args.ns, "frames": len(ms), "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
                "max_ms": round(max(ms), 3), "library": "RT_LIB_OVERRIDE" if os.environ.get("RT_LIB_OVERRIDE") else "this build"}
        if hasattr(ds, "cost_map") and hasattr(art.rt_lib(), "rt_debug_cost_map"):
            line["parts_of_the_last_frame"] = ds.cost_map()[2]
        ds.close()
        print(json.dumps(line))
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
        return

    # ---- (a) the kernel
    ds = art.DeviceScene(hs)
    f4 = hs.frame(nx=nx, ny=ny, ns=4, gamma=1.0)
    cams = [orbited(0.0, nx, ny), orbited(3.0, nx, ny)]
    host = []
    for cam in cams:
        ds.set_camera(cam)
        color, _ = ds.render(f4)
        host.append(dict(ds.render_aov(f4, ids=True), color=color))
    t = [{k: torch.from_numpy(v).to(dev) for k, v in h.items()} for h in host]
    first = art.reproject(t[0]["color"], t[0]["depth"], t[0]["alpha"], cams[0], cams[0])
    out, out_len = torch.empty_like(first.out), torch.empty_like(first.length)
    motion = torch.empty((ny, nx, 2), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    base = dict(history=first.out, history_len=first.length, prev_depth=t[0]["depth"], prev_alpha=t[0]["alpha"], out=out, out_len=out_len,
                stream=stream, blocking=False)
    guides = dict(normal=t[1]["normal"], prim=t[1]["prim"], prev_normal=t[0]["normal"], prev_prim=t[0]["prim"], motion=motion)
    if args.kernel_loop:
        ws = torch.empty(art.denoise_workspace_bytes(nx, ny), dtype=torch.uint8, device=dev)
        art.set_option("denoise_lds", 0)
        for _ in range(args.kernel_loop):
            art.reproject(t[1]["color"], t[1]["depth"], t[1]["alpha"], cams[1], cams[0], **dict(base, **guides))
            art.reproject(t[1]["color"], t[1]["depth"], t[1]["alpha"], cams[1], cams[0], **base)
            art.denoise(t[1]["color"], t[1]["albedo"], t[1]["normal"], t[1]["depth"], out=out, workspace=ws, stream=stream, blocking=False,
                        **dict(art.DENOISE_DEFAULTS, iterations=3))
        torch.cuda.synchronize()
        art.reset_options()
        ds.close()
        return
    for name, kw, per_pixel in (("all_guides", dict(base, **guides), 30), ("no_guides", base, 22)):
        ms = median_ms(lambda: art.reproject(t[1]["color"], t[1]["depth"], t[1]["alpha"], cams[1], cams[0], **kw))
        src = torch.empty(nx * ny * per_pixel, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy = median_ms(lambda: dst.copy_(src))
        found = float((out_len > 1).float().mean().item())
        lines.append({"what": "rt_reproject", "config": name, "nx": nx, "ny": ny, "median_ms": round(ms[0], 4), "min_ms": round(ms[1], 4),
                      "max_ms": round(ms[2], 4), "copy_ms": round(copy[0], 4), "copy_bytes_per_pixel_moved": 2 * per_pixel,
                      "over_copy": round(ms[0] / copy[0], 2), "pixels_with_history": round(found, 4)})
    art.set_option("denoise_lds", 0)
    ws = torch.empty(art.denoise_workspace_bytes(nx, ny), dtype=torch.uint8, device=dev)
    totals = [median_ms(lambda: art.denoise(t[1]["color"], t[1]["albedo"], t[1]["normal"], t[1]["depth"], out=out, workspace=ws, stream=stream,
                                            blocking=False, **dict(art.DENOISE_DEFAULTS, iterations=k)))[0] for k in (1, 2, 3)]
    art.reset_options()
    lines.append({"what": "rt_denoise unstaged iteration", "nx": nx, "ny": ny, "totals_ms_K1_K2_K3": [round(x, 4) for x in totals],
                  "iteration_ms_s2": round(totals[1] - totals[0], 4), "iteration_ms_s4": round(totals[2] - totals[1], 4),
                  "reproject_all_guides_over_iteration_s2": round(lines[0]["median_ms"] / (totals[1] - totals[0]), 3)})
    ds.close()

    # ---- (b) the stale prior
    cam = orbited(20.0, nx, ny)
    moved = art.HostScene("random_scene", nx, ny)
    moved.desc.camera = cam
    t0 = time.perf_counter()
    scenes = {"fresh": art.DeviceScene(moved)}
    create_ms = (time.perf_counter() - t0) * 1e3
    set_ms = {}
    for name, recal in (("stale", False), ("recalibrated", True)):
        scenes[name] = art.DeviceScene(hs)
        t0 = time.perf_counter()
        scenes[name].set_camera(cam, recalibrate=recal)
        set_ms[name] = (time.perf_counter() - t0) * 1e3
    f = hs.frame(nx=nx, ny=ny, ns=args.ns)
    fb = torch.empty((ny, nx, 3), dtype=torch.float32, device=dev)
    ms = {k: [] for k in scenes}
    rays = {}
    for it in range(args.frames + 1):           # the first round warms up
        for name, s in scenes.items():
            _, st = s.render(f, out=fb.data_ptr())
            rays[name] = st.rays
            if it:
                ms[name].append(st.ms_render)
    assert len(set(rays.values())) == 1, rays
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines.append({"what": "rt_render after a 20 degree set_camera", "scene": "random_scene", "nx": nx, "ny": ny, "ns": args.ns, "frames": args.frames,
                  "median_ms": {k: round(v, 3) for k, v in med.items()}, "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
                  "max_ms": {k: round(max(v), 3) for k, v in ms.items()}, "stale_over_fresh": round(med["stale"] / med["fresh"], 4),
                  "recalibrated_over_fresh": round(med["recalibrated"] / med["fresh"], 4), "rays": rays["fresh"],
                  "host_ms": {"rt_scene_create": round(create_ms, 2), "set_camera": round(set_ms["stale"], 3),
                              "set_camera_recalibrate": round(set_ms["recalibrated"], 3)}})
    for s in scenes.values():
        s.close()
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
