// rt_kernel_radiance.hip -- rt_radiance_rays (include/rt_abi.h): the reference's color() (main.cu:52-94) along caller-supplied
// rays, ns samples per query.  Internal to librt_mi355x.so; launched by rt_abi.hip.
//
// One query per lane, persistent workgroups: each workgroup stages the scene into LDS once (stage_scene) and then strides
// over the batch.  A lane keeps its whole query in registers -- the XORWOW state, the sample and bounce counters, the
// path's throughput and radiance, the colour sum, the walk's state -- and runs samples x bounces as one state machine:
// every trip of the loop is one node visit for the lanes that are walking and, for the lanes whose walk has just ended,
// the hit record, the material and what follows (the next bounce, the next sample, or the result and the next query).
// Path lengths range from 1 to 50 * ns rays, so a lane that finishes writes its result and loads its next query at once,
// without waiting for its wave.  No atomics, no inter-workgroup communication: the ray count is per query.
//
// A query is the single pixel of a 1 x 1 frame of a degenerate camera (include/rt_abi.h), so each sample first draws what
// a render sample draws before its path (rt_kernel_pixel.hip: two jitter uniforms, camera_get_ray's lens-disk loop and its
// shutter uniform) and discards it.
#include "rt_device_funcs.h"

namespace {

// One node visit of the walk for a ray with the window (0.001, best.t): bvh_node::hit (bvh.cuh:95-106) with the render
// kernels' guards on the faster box tests, as rt_kernel_trace.hip's trace_step.  `loose` (every 1/d component finite and
// loose_ok): interior boxes take the widened one-fma form and a leaf's own box is tested again exactly before its object;
// otherwise (a zero direction component) the reference's own slab form everywhere.  Returns the next node.
// Twin of trace_step<SPHERES_ONLY, false> there with tmin fixed: a change to one belongs in the other (kept apart so that
// rt_kernel_trace.hip compiles to the assembly it had).
template <bool SPHERES_ONLY>
DEV int walk_step(const SceneView& sc, const float4* nodes4, int node, const Ray& r, const f3 inv, const LooseRay& lr, bool loose,
                  HitInfo& best) {
    const float tmin = 0.001f;   // main.cu:57
    const float4 a = nodes4[2 * node], b = nodes4[2 * node + 1];
    const bool pass = loose ? slab_test_loose(a, b, inv, lr, tmin, best.t) : slab_test(a, b, r.o, inv, tmin, best.t);
    const int32_t link = __float_as_int(b.w), nskip = __float_as_int(a.w);   // rt_device.h, RT_NODE_SKIP
    const int next = ~((pass && link < 0) ? link : nskip);
    if (pass && link >= 0 && (!loose || slab_test_finite(a, b, r.o, inv, tmin, best.t))) leaf_test<SPHERES_ONLY>(sc, link, r, tmin, best);
    return next;
}

// the miss term of color() (main.cu:59-65): miss_color() for a batch's background
DEV f3 miss_term(const rt_radiance_params& rp, const Ray& r) {
    f3 bg = mk3(rp.background[0], rp.background[1], rp.background[2]);
    if (rp.use_gradient_bg) {
        const f3 ud = unit_vector(r.d);
        const float t = 0.5f * (ud.y + 1.0f);
        bg = mk3(fmaf(t, 0.5f, 1.0f - t), fmaf(t, 0.7f, 1.0f - t), (1.0f - t) + t);
    }
    return bg;
}

template <bool SPHERES_ONLY, int TEX, int LDS_MODE>
__global__ void __launch_bounds__(RT_RADIANCE_THREADS) rt_radiance_kernel(rt_scene_dev sd, rt_radiance_params rp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const SceneView sc = stage_scene<LDS_MODE>(sd, lds);
    const float4* nodes4 = reinterpret_cast<const float4*>(sc.nodes);
    const int nn = sc.n_nodes;
    const int64_t n = rp.n, stride = (int64_t)gridDim.x * blockDim.x;
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;

    rt_xorwow g;
    Ray q, cur;                  // the query's ray; the path's current ray
    f3 inv;
    LooseRay lr;
    bool loose = false;
    HitInfo best;
    int node = nn, sample = 0, bounce = 0;
    uint32_t rays = 0;
    f3 throughput, radiance, col;

    auto start_walk = [&]() {    // world->hit for `cur` (main.cu:57)
        ++rays;
        best.t = FLT_MAX; best.prim = -1; best.inst = -1;
        inv = mk3(1.0f / cur.d.x, 1.0f / cur.d.y, 1.0f / cur.d.z);
        loose = inv_is_finite(inv) && loose_ok(inv, cur.o, sd.bound);
        lr = loose_setup(inv, cur.o, sd.bound);
        node = 0;
    };
    auto start_sample = [&]() {
        // what a render sample draws before its path (rt_kernel_pixel.hip, camera_get_ray), discarded: with the degenerate
        // camera they select the same ray whatever they are
        (void)rt_xorwow_uniform(g);
        (void)rt_xorwow_uniform(g);
        f3 p;
        do {
            const float a = rt_xorwow_uniform(g);
            const float b = rt_xorwow_uniform(g);
            p = 2.0f * mk3(a, b, 0.0f) - mk3(1.0f, 1.0f, 0.0f);
        } while (dot(p, p) >= 1.0f);
        (void)rt_xorwow_uniform(g);
        cur = q;
        throughput = mk3(1, 1, 1); radiance = mk3(0, 0, 0);
        bounce = 0;
        start_walk();
    };
    // the lane's next query with a ray that can be walked; the others (a NaN or infinite component, the zero direction) get
    // zeros and no rays here, before any draw: quad_test and medium_test would accept a NaN t, and the box forms disagree on
    // NaN, so the walk taken would decide the answer (rt_kernel_trace.hip)
    auto begin = [&]() {
        node = nn;
        for (; idx < n; idx += stride) {
            q.o = ld3(rp.origins + 3 * idx);
            q.d = ld3(rp.directions + 3 * idx);
            q.tm = rp.times ? rp.times[idx] : 0.0f;
            const bool finite = isfinite(q.o.x) && isfinite(q.o.y) && isfinite(q.o.z) && isfinite(q.d.x) && isfinite(q.d.y) &&
                                isfinite(q.d.z) && isfinite(q.tm);
            if (finite && (q.d.x != 0.0f || q.d.y != 0.0f || q.d.z != 0.0f)) break;
            rp.rgb_out[3 * idx] = 0.0f; rp.rgb_out[3 * idx + 1] = 0.0f; rp.rgb_out[3 * idx + 2] = 0.0f;
            if (rp.rays_out) rp.rays_out[idx] = 0u;
        }
        if (idx >= n) return;
        rt_xorwow_seed(g, rp.seeds ? rp.seeds[idx] : rp.seed_base + (uint64_t)idx);   // render_init, main.cu:101-104
        col = mk3(0, 0, 0);
        sample = 0; rays = 0;
        start_sample();
    };

    begin();
    while (__ballot(idx < n) != 0ull) {
        if (node < nn) node = walk_step<SPHERES_ONLY>(sc, nodes4, node, cur, inv, lr, loose, best);
        if (idx < n && node >= nn) {   // this ray's walk is over: the rest of color()'s loop body (main.cu:57-92)
            bool path_over;
            if (best.prim < 0) {
                radiance = fma3(throughput, miss_term(rp, cur), radiance);
                path_over = true;
            } else {
                const HitRec rec = resolve_hit<SPHERES_ONLY, TEX == 2>(sc, cur, best);
                f3 emitted, attenuation;
                Ray scattered;
                const bool go_on = shade<TEX>(sc, cur, rec, g, emitted, attenuation, scattered);
                radiance = fma3(throughput, emitted, radiance);
                path_over = !go_on;
                if (go_on) {
                    throughput = throughput * attenuation;
                    cur = scattered;
                    path_over = ++bounce == 50;   // main.cu:54
                }
            }
            if (!path_over) {
                start_walk();
            } else {
                col = col + radiance;
                if (++sample < rp.ns) {
                    start_sample();
                } else {
                    const float k = (float)(1.0 / (double)(float)rp.ns);   // store_pixel: vec3::operator/=(float), vec3.cuh:145-153
                    rp.rgb_out[3 * idx] = col.x * k; rp.rgb_out[3 * idx + 1] = col.y * k; rp.rgb_out[3 * idx + 2] = col.z * k;
                    if (rp.rays_out) rp.rays_out[idx] = rays;
                    idx += stride;
                    begin();
                }
            }
        }
    }
}

template <bool SO, int TEX, int LM>
hipError_t set_lds(size_t lds) {
    if (lds <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&rt_radiance_kernel<SO, TEX, LM>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

template <bool SO, int TEX, int LM>
struct Launch {
    static hipError_t run(const rt_scene_dev* sd, const rt_radiance_params* rp, dim3 grid, size_t lds, hipStream_t st) {
        const hipError_t e = set_lds<SO, TEX, LM>(lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((rt_radiance_kernel<SO, TEX, LM>), grid, dim3(RT_RADIANCE_THREADS), lds, st, *sd, *rp);
        return hipGetLastError();
    }
};
template <bool SO, int TEX, int LM>
struct Occupancy {
    static hipError_t run(size_t lds, int* blocks) {
        const hipError_t e = set_lds<SO, TEX, LM>(lds);
        if (e != hipSuccess) return e;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void*>(&rt_radiance_kernel<SO, TEX, LM>),
                                                            RT_RADIANCE_THREADS, lds);
    }
};

// every instantiation behind one switch: F<SO, TEX, LM>::run(args...)
template <template <bool, int, int> class F, bool SO, int TEX, typename... A>
hipError_t dispatch_lds(int lds_mode, A... args) {
    if (lds_mode == 2) return F<SO, TEX, 2>::run(args...);
    if (lds_mode == 1) return F<SO, TEX, 1>::run(args...);
    return F<SO, TEX, 0>::run(args...);
}
template <template <bool, int, int> class F, typename... A>
hipError_t dispatch(bool spheres_only, int tex_level, int lds_mode, A... args) {
    if (spheres_only) {
        if (tex_level == 0) return dispatch_lds<F, true, 0>(lds_mode, args...);
        if (tex_level == 1) return dispatch_lds<F, true, 1>(lds_mode, args...);
        return dispatch_lds<F, true, 2>(lds_mode, args...);
    }
    if (tex_level == 0) return dispatch_lds<F, false, 0>(lds_mode, args...);
    if (tex_level == 1) return dispatch_lds<F, false, 1>(lds_mode, args...);
    return dispatch_lds<F, false, 2>(lds_mode, args...);
}

}  // namespace

hipError_t rt_launch_radiance(bool spheres_only, int tex_level, int lds_mode, const rt_scene_dev& sd, const rt_radiance_params& rp,
                              dim3 grid, size_t lds, hipStream_t st) {
    return dispatch<Launch>(spheres_only, tex_level, lds_mode, &sd, &rp, grid, lds, st);
}

hipError_t rt_radiance_occupancy(bool spheres_only, int tex_level, int lds_mode, size_t lds, int* blocks_per_cu) {
    return dispatch<Occupancy>(spheres_only, tex_level, lds_mode, lds, blocks_per_cu);
}
