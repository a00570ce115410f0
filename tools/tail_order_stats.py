#!/usr/bin/env python3
"""What ordering the tail hand-off queue can save, measured before anything is timed: renders FRAMES (default 3)
frames like tools/one_frame.py, reads the last frame's queue (rt_debug_handoff_queue), computes every entry's remaining-work key
(rays, csrc/rt_handoff_order.h) and simulates the tail launch's waves pulling entries in push order, in the order the tail launch
was given, and in exact key order.  One JSON line: the key's distribution and the three makespans in rays.  With TAIL_MS=<the tail
launch's duration in the kernel trace of the same configuration> it adds the tail's microseconds per ray = TAIL_MS / makespan
of the order that launch was served in.
SCENE / NX / NY / NS select the frame, RT_OPTS=key=value,... the knobs (handoff_order=0: the tail is served in push order)."""
import heapq, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import accelerated_ray_tracer_amd as art


def makespan(jobs, servers):
    """List scheduling: every server takes the next job of the list when it falls idle."""
    free = [0] * min(servers, max(len(jobs), 1))
    heapq.heapify(free)
    end = 0
    for j in jobs:
        t = heapq.heappop(free) + int(j)
        end = max(end, t)
        heapq.heappush(free, t)
    return end


art.init(0)
for kv in filter(None, os.environ.get("RT_OPTS", "").split(",")):
    k, v = kv.split("="); art.set_option(k, int(v))
scene, nx, ny, ns = os.environ.get("SCENE", "random_scene"), int(os.environ.get("NX", "1200")), int(os.environ.get("NY", "800")), int(os.environ.get("NS", "500"))
img, iw, ih = art.default_texture(scene)
hs = art.HostScene(scene, nx, ny, img, iw, ih)
ds = art.DeviceScene(hs)
f = hs.frame(nx=nx, ny=ny, ns=ns)
buf = torch.zeros((ny, nx, 3), dtype=torch.float32, device="cuda")
for _ in range(int(os.environ.get("FRAMES", "3"))):
    _, st = ds.render(f, out=buf.data_ptr(), blocking=True)
entries, costs, served, info = ds.handoff_queue()
parts = ds.cost_map()[2]
# (the last part's parked costs count from sample 0: a one-part frame starts there, a later part resumes pixels parked with all their rays)
keys = art.handoff_order_key(entries, costs, 0, ns)
key_of = dict(zip(entries.tolist(), keys.tolist()))
served_keys = [key_of[e] for e in served.tolist()]
waves = info["min"] // art.HANDOFF_ORDER_MIN_PER_WAVE if info["min"] else int(os.environ.get("TAIL_WAVES", "3072"))
k = np.array(keys.tolist(), np.float64)
to_go = ns - (entries >> np.uint64(32)).astype(np.int64)
out = dict(scene=scene, nx=nx, ny=ny, ns=ns, parts=parts, ms_render=round(st.ms_render, 3), entries=len(entries), tail_waves=waves,
           ordered_by_library=info["ordered"] and info["min"] <= len(entries) <= info["max"],
           samples_to_go=dict(mean=round(float(to_go.mean()), 1), max=int(to_go.max())) if len(entries) else None,
           key_rays=dict(sum=int(k.sum()), mean=round(float(k.mean()), 1), p50=int(np.percentile(k, 50)), p90=int(np.percentile(k, 90)),
                         p99=int(np.percentile(k, 99)), max=int(k.max()), mean_load_per_wave=round(float(k.sum()) / waves, 1)) if len(entries) else None,
           makespan_rays=dict(push_order=makespan(keys.tolist(), waves), as_served=makespan(served_keys, waves),
                              key_order=makespan(sorted(keys.tolist(), reverse=True), waves)))
if os.environ.get("TAIL_MS") and out["makespan_rays"]["as_served"]:
    out["tail_ms_traced"] = float(os.environ["TAIL_MS"])
    out["tail_us_per_ray"] = round(1e3 * out["tail_ms_traced"] / out["makespan_rays"]["as_served"], 3)
print(json.dumps(out), flush=True)
