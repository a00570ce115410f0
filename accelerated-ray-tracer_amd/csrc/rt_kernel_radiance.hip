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
#include "rt_kernel_query.h"
#include "rt_launch.h"

namespace {

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

    // world->hit for `cur` (main.cu:57); walk_start (rt_kernel_query.h) written out: calling it changes this kernel's
    // instruction stream
    auto start_walk = [&]() {
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
    // zeros and no rays here, before any draw (ray_is_finite)
    auto begin = [&]() {
        node = nn;
        for (; idx < n; idx += stride) {
            q.o = ld3(rp.origins + 3 * idx);
            q.d = ld3(rp.directions + 3 * idx);
            q.tm = rp.times ? rp.times[idx] : 0.0f;
            if (ray_is_finite(q) && (q.d.x != 0.0f || q.d.y != 0.0f || q.d.z != 0.0f)) break;
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
        if (node < nn) node = walk_step<SPHERES_ONLY, false>(sc, nodes4, node, cur, inv, lr, loose, 0.001f, best);   // main.cu:57
        if (idx < n && node >= nn) {   // this ray's walk is over: the rest of color()'s loop body (main.cu:57-92)
            bool path_over;
            if (best.prim < 0) {
                radiance = fma3(throughput, miss_color(rp, cur), radiance);
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

using Kernel = void (*)(rt_scene_dev, rt_radiance_params);

template <bool SO, int TEX>
Kernel pick_lds(int lds_mode) {
    if (lds_mode == 2) return rt_radiance_kernel<SO, TEX, 2>;
    if (lds_mode == 1) return rt_radiance_kernel<SO, TEX, 1>;
    return rt_radiance_kernel<SO, TEX, 0>;
}
template <bool SO>
Kernel pick_tex(int tex_level, int lds_mode) {
    if (tex_level == 0) return pick_lds<SO, 0>(lds_mode);
    if (tex_level == 1) return pick_lds<SO, 1>(lds_mode);
    return pick_lds<SO, 2>(lds_mode);
}
Kernel pick(bool spheres_only, int tex_level, int lds_mode) {
    return spheres_only ? pick_tex<true>(tex_level, lds_mode) : pick_tex<false>(tex_level, lds_mode);
}

}  // namespace

hipError_t rt_launch_radiance(bool spheres_only, int tex_level, int lds_mode, const rt_scene_dev& sd, const rt_radiance_params& rp,
                              dim3 grid, size_t lds, hipStream_t st) {
    return rt_launch_kernel(pick(spheres_only, tex_level, lds_mode), dim3(RT_RADIANCE_THREADS), grid, lds, st, sd, rp);
}

hipError_t rt_radiance_occupancy(bool spheres_only, int tex_level, int lds_mode, size_t lds, int* blocks_per_cu) {
    return rt_kernel_occupancy(pick(spheres_only, tex_level, lds_mode), RT_RADIANCE_THREADS, lds, blocks_per_cu);
}
