// rt_kernel_trace.hip -- rt_trace_rays (include/rt_abi.h): closest-hit and any-hit queries for caller-supplied rays,
// walked with the render kernels' BVH walk and leaf tests.  Internal to librt_mi355x.so; launched by rt_abi.hip.
//
// One ray per lane, persistent workgroups: each workgroup stages the scene into LDS once (stage_scene) and then strides
// over the batch.  A lane whose ray is finished writes its result and loads its next ray at once, without waiting for
// the rest of its wave (incoherent rays end at very different times); only when a hit record is requested does a wave
// finish its rays together, so that the record code -- a transform, a division, acos / atan2 in double -- runs once per
// 64 rays rather than once per finishing lane.  No atomics, no inter-workgroup communication.
#include "rt_device_funcs.h"

namespace {

// One node visit of the walk for a ray with the window (tmin, best.t): bvh_node::hit (bvh.cuh:95-106) as trace() walks it,
// with the render kernels' guards on the faster box tests.  `loose` (every 1/d component finite and loose_ok): interior
// boxes take the widened one-fma form, a superset of aabb::hit's passes, and a leaf's own box is tested again exactly
// (slab_test_finite) before its object -- the walk then reaches exactly the objects the reference reaches (rt_device_funcs.h,
// "the walk loop's box test").  Otherwise (a zero direction component): the reference's own
// slab form everywhere.  Returns the next node; for ANY it returns n_nodes at the first accepted leaf.
template <bool SPHERES_ONLY, bool ANY>
DEV int trace_step(const SceneView& sc, const float4* nodes4, int node, const Ray& r, const f3 inv, const LooseRay& lr, bool loose,
                   float tmin, HitInfo& best) {
    const float4 a = nodes4[2 * node], b = nodes4[2 * node + 1];
    const bool pass = loose ? slab_test_loose(a, b, inv, lr, tmin, best.t) : slab_test(a, b, r.o, inv, tmin, best.t);
    // device encoding of the links (rt_device.h, RT_NODE_SKIP): a.w = ~skip; b.w = ~(node + 1) inside, the object id at a leaf
    const int32_t link = __float_as_int(b.w), nskip = __float_as_int(a.w);
    int next = ~((pass && link < 0) ? link : nskip);
    if (pass && link >= 0 && (!loose || slab_test_finite(a, b, r.o, inv, tmin, best.t))) {
        leaf_test<SPHERES_ONLY>(sc, link, r, tmin, best);
        if (ANY && best.prim >= 0) next = sc.n_nodes;
    }
    return next;
}

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
        best.t = tp.tmax ? tp.tmax[idx] : FLT_MAX;
        best.prim = -1; best.inst = -1;
        inv = mk3(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
        loose = inv_is_finite(inv) && loose_ok(inv, r.o, sd.bound);
        lr = loose_setup(inv, r.o, sd.bound);
        // a NaN tmax is a miss: sphere_test would reject every root under it, but quad_test's `t > tmax` and medium_test's
        // clamp do not see a NaN, so the walk is not entered at all.  So is a ray with a non-finite origin, direction or
        // time: quad_test and medium_test would accept a NaN t, and the box forms disagree on NaN (fminf / fmaxf drop it,
        // the ternaries keep it), so the walk taken would decide the answer.
        const bool finite = isfinite(r.o.x) && isfinite(r.o.y) && isfinite(r.o.z) && isfinite(r.d.x) && isfinite(r.d.y) &&
                            isfinite(r.d.z) && isfinite(r.tm);
        node = (finite && best.t == best.t) ? 0 : nn;
    };
    begin();
    while (__ballot(idx < n) != 0ull) {
        if (node < nn) node = trace_step<SPHERES_ONLY, ANY>(sc, nodes4, node, r, inv, lr, loose, tmin, best);
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

template <bool SO, int LM, bool ANY, bool REC>
hipError_t launch_one(const rt_scene_dev& sd, const rt_trace_params& tp, dim3 grid, size_t lds, hipStream_t st) {
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rt_trace_kernel<SO, LM, ANY, REC>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((rt_trace_kernel<SO, LM, ANY, REC>), grid, dim3(RT_TRACE_THREADS), lds, st, sd, tp);
    return hipGetLastError();
}

template <bool SO, int LM, bool ANY, bool REC>
hipError_t occupancy_one(size_t lds, int* blocks) {
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rt_trace_kernel<SO, LM, ANY, REC>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void*>(&rt_trace_kernel<SO, LM, ANY, REC>),
                                                        RT_TRACE_THREADS, lds);
}

// every instantiation behind one switch: F<SO, LM, ANY, REC>::run(args...)
template <template <bool, int, bool, bool> class F, bool SO, typename... A>
hipError_t dispatch_lds(int lds_mode, bool any, bool record, A... args) {
#define RT_TRACE_CASE(LM)                                                        \
    do {                                                                         \
        if (any) return F<SO, LM, true, false>::run(args...);                   \
        if (record) return F<SO, LM, false, true>::run(args...);                \
        return F<SO, LM, false, false>::run(args...);                           \
    } while (0)
    if (lds_mode == 2) RT_TRACE_CASE(2);
    if (lds_mode == 1) RT_TRACE_CASE(1);
    RT_TRACE_CASE(0);
#undef RT_TRACE_CASE
}
template <bool SO, int LM, bool ANY, bool REC>
struct Launch { static hipError_t run(const rt_scene_dev* sd, const rt_trace_params* tp, dim3 grid, size_t lds, hipStream_t st) { return launch_one<SO, LM, ANY, REC>(*sd, *tp, grid, lds, st); } };
template <bool SO, int LM, bool ANY, bool REC>
struct Occupancy { static hipError_t run(size_t lds, int* blocks) { return occupancy_one<SO, LM, ANY, REC>(lds, blocks); } };

}  // namespace

hipError_t rt_launch_trace(bool spheres_only, int lds_mode, const rt_scene_dev& sd, const rt_trace_params& tp, dim3 grid, size_t lds,
                           hipStream_t st) {
    const bool any = tp.hit_out != nullptr, record = tp.record != 0;
    if (spheres_only) return dispatch_lds<Launch, true>(lds_mode, any, record, &sd, &tp, grid, lds, st);
    return dispatch_lds<Launch, false>(lds_mode, any, record, &sd, &tp, grid, lds, st);
}

hipError_t rt_trace_occupancy(bool spheres_only, int lds_mode, bool any, bool record, size_t lds, int* blocks_per_cu) {
    if (spheres_only) return dispatch_lds<Occupancy, true>(lds_mode, any, record, lds, blocks_per_cu);
    return dispatch_lds<Occupancy, false>(lds_mode, any, record, lds, blocks_per_cu);
}
