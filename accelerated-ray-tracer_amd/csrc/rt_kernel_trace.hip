// rt_kernel_trace.hip -- rt_trace_rays (include/rt_abi.h): closest-hit and any-hit queries for caller-supplied rays,
// walked with the render kernels' BVH walk and leaf tests.  Internal to librt_mi355x.so; launched by rt_abi.hip.
//
// One ray per lane, persistent workgroups: each workgroup stages the scene into LDS once (stage_scene) and then strides
// over the batch.  A lane whose ray is finished writes its result and loads its next ray at once, without waiting for
// the rest of its wave (incoherent rays end at very different times); only when a hit record is requested does a wave
// finish its rays together, so that the record code -- a transform, a division, acos / atan2 in double -- runs once per
// 64 rays rather than once per finishing lane.  No atomics, no inter-workgroup communication.
#include "rt_kernel_query.h"
#include "rt_launch.h"

namespace {

// the hit record of a closest hit: resolve_hit() as the render computes it, and the sphere's (u, v) always (the render
// computes them only where a material reads them) -- get_sphere_uv of the object-space outward normal, sphere.cuh:42-49
template <bool SPHERES_ONLY>
DEV HitRec trace_record(const SceneView& sc, const Ray& r, const HitInfo& h) {
    HitRec rec = resolve_hit<SPHERES_ONLY, false>(sc, r, h);
    if (SPHERES_ONLY || RT_PRIM_KIND(h.prim) == RT_PRIM_SPHERE) {
        const Ray q = (!SPHERES_ONLY && h.inst >= 0) ? to_object_space(sc.instances[h.inst], r) : r;
        const rt_sphere s = sc.spheres[RT_PRIM_INDEX(h.prim)];
        const f3 cc = fma3(q.tm, ld3(s.vel), ld3(s.c0));
        sphere_uv(sdiv(ray_at(q, h.t) - cc, s.radius), rec.u, rec.v);
    }
    return rec;
}

template <bool SPHERES_ONLY, int LDS_MODE, bool ANY, bool RECORD>
__global__ void __launch_bounds__(RT_TRACE_THREADS) rt_trace_kernel(rt_scene_dev sd, rt_trace_params tp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const SceneView sc = stage_scene<LDS_MODE>(sd, lds);
    const float4* nodes4 = reinterpret_cast<const float4*>(sc.nodes);
    const int nn = sc.n_nodes;
    const float tmin = tp.tmin;
    const int64_t n = tp.n, stride = (int64_t)gridDim.x * blockDim.x;
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;

    Ray r;
    f3 inv;
    LooseRay lr;
    bool loose = false;
    HitInfo best;
    int node = nn;
    auto begin = [&]() {
        node = nn;
        if (idx >= n) return;
        r.o = ld3(tp.origins + 3 * idx);
        r.d = ld3(tp.directions + 3 * idx);
        r.tm = tp.times ? tp.times[idx] : 0.0f;
        // walk_start (rt_kernel_query.h) written out: calling it changes this kernel's instruction stream
        best.t = tp.tmax ? tp.tmax[idx] : FLT_MAX;
        best.prim = -1; best.inst = -1;
        inv = mk3(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
        loose = inv_is_finite(inv) && loose_ok(inv, r.o, sd.bound);
        lr = loose_setup(inv, r.o, sd.bound);
        // a NaN tmax is a miss: sphere_test would reject every root under it, but quad_test's `t > tmax` and medium_test's
        // clamp do not see a NaN, so the walk is not entered at all.  So is a ray that is not finite (ray_is_finite).
        node = (ray_is_finite(r) && best.t == best.t) ? 0 : nn;
    };
    begin();
    while (__ballot(idx < n) != 0ull) {
        if (node < nn) node = walk_step<SPHERES_ONLY, ANY>(sc, nodes4, node, r, inv, lr, loose, tmin, best);
        const bool finish = RECORD ? __ballot(idx < n && node < nn) == 0ull : (idx < n && node >= nn);
        if (finish) {
            if (idx < n) {
                const bool hit = best.prim >= 0;
                if (ANY) {
                    tp.hit_out[idx] = hit ? 1 : 0;
                } else {
                    tp.t_out[idx] = hit ? best.t : FLT_MAX;
                    tp.prim_out[idx] = best.prim;
                    if (tp.inst_out) tp.inst_out[idx] = best.inst;
                    if (RECORD) {
                        if (hit) {
                            const HitRec rec = trace_record<SPHERES_ONLY>(sc, r, best);
                            if (tp.point_out) { tp.point_out[3 * idx] = rec.p.x; tp.point_out[3 * idx + 1] = rec.p.y; tp.point_out[3 * idx + 2] = rec.p.z; }
                            if (tp.normal_out) { tp.normal_out[3 * idx] = rec.n.x; tp.normal_out[3 * idx + 1] = rec.n.y; tp.normal_out[3 * idx + 2] = rec.n.z; }
                            if (tp.uv_out) { tp.uv_out[2 * idx] = rec.u; tp.uv_out[2 * idx + 1] = rec.v; }
                            if (tp.mat_out) tp.mat_out[idx] = rec.mat;
                        } else {   // a miss: zeros, material -1
                            if (tp.point_out) { tp.point_out[3 * idx] = 0.0f; tp.point_out[3 * idx + 1] = 0.0f; tp.point_out[3 * idx + 2] = 0.0f; }
                            if (tp.normal_out) { tp.normal_out[3 * idx] = 0.0f; tp.normal_out[3 * idx + 1] = 0.0f; tp.normal_out[3 * idx + 2] = 0.0f; }
                            if (tp.uv_out) { tp.uv_out[2 * idx] = 0.0f; tp.uv_out[2 * idx + 1] = 0.0f; }
                            if (tp.mat_out) tp.mat_out[idx] = -1;
                        }
                    }
                }
            }
            idx += stride;
            begin();
        }
    }
}

using Kernel = void (*)(rt_scene_dev, rt_trace_params);

// the instantiation of a launch: any-hit before record
template <bool SO, int LM>
Kernel pick_mode(bool any, bool record) {
    if (any) return rt_trace_kernel<SO, LM, true, false>;
    if (record) return rt_trace_kernel<SO, LM, false, true>;
    return rt_trace_kernel<SO, LM, false, false>;
}
template <bool SO>
Kernel pick_lds(int lds_mode, bool any, bool record) {
    if (lds_mode == 2) return pick_mode<SO, 2>(any, record);
    if (lds_mode == 1) return pick_mode<SO, 1>(any, record);
    return pick_mode<SO, 0>(any, record);
}
Kernel pick(bool spheres_only, int lds_mode, bool any, bool record) {
    return spheres_only ? pick_lds<true>(lds_mode, any, record) : pick_lds<false>(lds_mode, any, record);
}

}  // namespace

hipError_t rt_launch_trace(bool spheres_only, int lds_mode, const rt_scene_dev& sd, const rt_trace_params& tp, dim3 grid, size_t lds,
                           hipStream_t st) {
    const Kernel kernel = pick(spheres_only, lds_mode, tp.hit_out != nullptr, tp.record != 0);
    return rt_launch_kernel(kernel, dim3(RT_TRACE_THREADS), grid, lds, st, sd, tp);
}

hipError_t rt_trace_occupancy(bool spheres_only, int lds_mode, bool any, bool record, size_t lds, int* blocks_per_cu) {
    return rt_kernel_occupancy(pick(spheres_only, lds_mode, any, record), RT_TRACE_THREADS, lds, blocks_per_cu);
}
