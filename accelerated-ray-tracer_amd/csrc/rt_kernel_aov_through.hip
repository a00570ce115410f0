// rt_kernel_aov_through.hip -- rt_render_aov_through (include/rt_abi.h): the feature buffers of a frame at the first
// NON-SPECULAR surface of every sample -- the primary rays rt_render_aov sends, each followed through mirrors and glass along
// a deterministic chain.  Internal to librt_mi355x.so; launched by rt_abi.hip.
//
// rt_kernel_aov.hip's state machine -- one pixel per lane, persistent workgroups, the scene staged in LDS once per workgroup,
// 8 x 8 pixel tiles of 64 consecutive work items -- with the chain's state added to what a lane keeps in registers: the tint,
// the number of followed bounces k, the primary hit's t, the sum of the later rays' t and |d0|.  Every trip of the loop is one
// node visit for the lanes that are walking; a lane whose walk has just ended resolves its hit and either sets up the chain's
// next ray in the same trip (a followed mirror or glass hit) or ends the sample as rt_kernel_aov.hip does.  The chain consumes
// no draw.  No atomics, no inter-workgroup communication.
//
// The arithmetic of the chain's directions is the contract's (include/rt_abi.h): binary32, one rounding per written operation,
// no FMA -- plain helpers below, not dot / reflect / refract of rt_device_funcs.h, which carry the renderer's contractions.
#include "rt_kernel_query.h"
#include "rt_launch.h"

namespace {

// rt_kernel_aov.hip's hit_albedo for a material already loaded
template <int TEX>
DEV f3 hit_albedo(const SceneView& sc, const rt_material& m, const HitRec& rec) {
    if (m.kind == RT_MAT_DIELECTRIC) return mk3(1.0f, 1.0f, 1.0f);
    if (TEX > 0 && m.kind != RT_MAT_METAL && m.tex >= 0) return texture_value<TEX>(sc, m.tex, rec.u, rec.v, rec.p);
    return ld3(m.albedo);
}

// the contract's plain arithmetic: every operation rounded once, nothing fused (the unit is built with -ffp-contract=off)
DEV float pdot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
DEV f3 mirror(f3 u, f3 n) {   // u - (2 dot(u, n)) n
    const float c2 = 2.0f * pdot(u, n);
    return mk3(u.x - c2 * n.x, u.y - c2 * n.y, u.z - c2 * n.z);
}
DEV f3 through_glass(f3 d, f3 u, f3 n, float ior) {
    const bool inside = pdot(d, n) > 0.0f;
    const f3 m = inside ? -n : n;
    const float e = inside ? ior : 1.0f / ior;
    const float dt = pdot(u, m);
    const float disc = 1.0f - (e * e) * (1.0f - dt * dt);
    if (disc > 0.0f) {
        const float s = sqrtf(disc);
        return mk3(e * (u.x - dt * m.x) - s * m.x, e * (u.y - dt * m.y) - s * m.y, e * (u.z - dt * m.z) - s * m.z);
    }
    return mirror(u, n);   // total internal reflection
}

template <bool SPHERES_ONLY, int TEX, int LDS_MODE>
__global__ void __launch_bounds__(RT_AOV_THREADS) rt_aov_through_kernel(rt_scene_dev sd, rt_aov_params ap, rt_aov_through_params tp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const SceneView sc = stage_scene<LDS_MODE>(sd, lds);
    const float4* nodes4 = reinterpret_cast<const float4*>(sc.nodes);
    const int nn = sc.n_nodes;
    // work items as rt_kernel_aov.hip cuts them: w = (tile << 6) | position in the tile, a wave always holds one whole tile
    const uint32_t items = ap.work_items, stride = gridDim.x * blockDim.x;
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    const bool want_albedo = ap.albedo != nullptr;
    const bool want_rec = want_albedo || ap.normal != nullptr || ap.mat != nullptr;   // (a hit that may be followed needs it too)
    const int max_bounces = tp.max_bounces;

    rt_xorwow g;
    Ray cur;
    f3 inv;
    LooseRay lr;
    bool loose = false;
    HitInfo best;
    int node = nn, sample = 0, i = 0, j = 0;
    size_t px = 0;               // lrow * nx + i: the pixel's place in every output
    f3 alb, nrm;
    float depth = 0.0f, alpha = 0.0f, thr = 0.0f;
    // the chain of the current sample
    f3 tint;
    int k = 0;
    float t0 = 0.0f, tsum = 0.0f, len0 = 1.0f;

    // world->hit for `cur` (main.cu:57); walk_start (rt_kernel_query.h) written out: calling it changes this kernel's
    // instruction stream
    auto start_walk = [&]() {
        best.t = FLT_MAX; best.prim = -1; best.inst = -1;
        inv = mk3(1.0f / cur.d.x, 1.0f / cur.d.y, 1.0f / cur.d.z);
        loose = inv_is_finite(inv) && loose_ok(inv, cur.o, sd.bound);
        lr = loose_setup(inv, cur.o, sd.bound);
        node = 0;
    };
    auto start_sample = [&]() {  // rt_kernel_pixel.hip: the sample's place in the pixel, then camera_get_ray's draws
        const float u = ((float)i + rt_xorwow_uniform(g)) / (float)ap.nx;
        const float v = ((float)j + rt_xorwow_uniform(g)) / (float)ap.ny;
        cur = camera_get_ray(sd.camera, u, v, g);
        tint = mk3(1.0f, 1.0f, 1.0f);
        k = 0; tsum = 0.0f;
        start_walk();
    };
    // the lane's next work item that is a pixel of the frame (tiles overhang its right and top edges): rt_kernel_aov.hip's begin,
    // with thr
    auto begin = [&]() {
        node = nn;
        int lrow = 0;
        for (; w < items; w += stride) {
            const uint32_t tile = w >> 6, within = w & 63u;
            i = (int)((tile % (uint32_t)ap.tiles_x) * 8u + (within & 7u));
            lrow = (int)((tile / (uint32_t)ap.tiles_x) * 8u + (within >> 3));
            if (i < ap.nx && lrow < ap.local_rows) break;
        }
        if (w >= items) return;
        const int t = lrow / ap.tile_rows;   // local_to_global_row
        j = (ap.tile_first + t * ap.tile_stride) * ap.tile_rows + (lrow - t * ap.tile_rows);
        px = (size_t)lrow * ap.nx + i;
        rt_xorwow_seed(g, ap.seed_base + (uint64_t)(j * ap.nx + i));   // render_init, main.cu:101-104
        alb = mk3(0, 0, 0); nrm = mk3(0, 0, 0);
        depth = 0.0f; alpha = 0.0f; thr = 0.0f;
        sample = 0;
        start_sample();
    };

    begin();
    while (__ballot(w < items) != 0ull) {
        if (node < nn) node = walk_step<SPHERES_ONLY, false>(sc, nodes4, node, cur, inv, lr, loose, 0.001f, best);   // main.cu:57
        if (w < items && node >= nn) {   // the walk of ray k is over
            const bool hit = best.prim >= 0;
            const bool may_follow = k < max_bounces && (SPHERES_ONLY || RT_PRIM_KIND(best.prim) != RT_PRIM_MEDIUM);
            bool follow = false;
            int32_t mat = -1;
            if (hit) {
                HitRec rec;
                rt_material m;
                m.kind = RT_MAT_LAMBERTIAN;
                if (want_rec || may_follow) {
                    // the sphere's (u, v) -- acos / atan2 in double -- only under a texture that reads it, and only for albedo
                    rec = (TEX == 2 && want_albedo) ? resolve_hit<SPHERES_ONLY, true>(sc, cur, best)
                                                    : resolve_hit<SPHERES_ONLY, false>(sc, cur, best);
                    mat = rec.mat;
                    m = sc.materials[rec.mat];
                }
                if (may_follow && (m.kind == RT_MAT_DIELECTRIC || (m.kind == RT_MAT_METAL && m.fuzz <= tp.fuzz_limit))) {
                    const float len = sqrtf(pdot(cur.d, cur.d));
                    const f3 u = mk3(cur.d.x / len, cur.d.y / len, cur.d.z / len);
                    f3 next;
                    if (m.kind == RT_MAT_METAL) {
                        next = mirror(u, rec.n);
                        follow = pdot(rec.n, next) > 0.0f;   // a mirror direction into the surface ends the chain here
                        if (follow) tint = tint * ld3(m.albedo);
                    } else {
                        next = through_glass(cur.d, u, rec.n, m.ior);
                        follow = true;
                    }
                    if (follow) {   // ray k + 1, set up in this trip
                        if (k == 0) { t0 = best.t; len0 = len; } else { tsum = tsum + best.t; }
                        ++k;
                        cur.o = rec.p; cur.d = next;
                        start_walk();
                        // a followed ray with a non-finite component is a miss, as rt_trace_rays decides it (an ior of 0, say)
                        if (!(isfinite(cur.o.x) && isfinite(cur.o.y) && isfinite(cur.o.z) && isfinite(next.x) && isfinite(next.y) && isfinite(next.z)))
                            node = nn;
                    }
                }
                if (!follow) {   // the terminal hit
                    if (want_rec) nrm = nrm + rec.n;
                    if (want_albedo) alb = alb + tint * hit_albedo<TEX>(sc, m, rec);
                    depth = depth + (k == 0 ? best.t : t0 + (tsum + best.t) / len0);
                    alpha = alpha + 1.0f;
                }
            } else if (want_albedo) {
                alb = alb + tint * miss_color(ap, cur);
            }
            if (!follow) {       // the sample's chain has ended
                if (k >= 1) thr = thr + 1.0f;
                if (sample == 0) {           // the ids and the bounce count are the first sample's
                    if (ap.prim) ap.prim[px] = best.prim;
                    if (ap.inst) ap.inst[px] = best.inst;
                    if (ap.mat) ap.mat[px] = mat;
                    if (tp.bounces) tp.bounces[px] = k;
                }
                if (++sample < ap.ns) {
                    start_sample();
                } else {
                    const float s = (float)(1.0 / (double)(float)ap.ns);   // store_pixel: vec3::operator/=(float), vec3.cuh:145-153
                    if (want_albedo) st3(ap.albedo + 3 * px, alb, s);
                    if (ap.normal) st3(ap.normal + 3 * px, nrm, s);
                    if (ap.depth) ap.depth[px] = depth * s;
                    if (ap.alpha) ap.alpha[px] = alpha * s;
                    if (tp.through) tp.through[px] = thr * s;
                    w += stride;
                    begin();
                }
            }
        }
    }
}

using Kernel = void (*)(rt_scene_dev, rt_aov_params, rt_aov_through_params);

template <bool SO, int TEX>
Kernel pick_lds(int lds_mode) {
    if (lds_mode == 2) return rt_aov_through_kernel<SO, TEX, 2>;
    if (lds_mode == 1) return rt_aov_through_kernel<SO, TEX, 1>;
    return rt_aov_through_kernel<SO, TEX, 0>;
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

hipError_t rt_launch_aov_through(bool spheres_only, int tex_level, int lds_mode, const rt_scene_dev& sd, const rt_aov_params& ap,
                                 const rt_aov_through_params& tp, dim3 grid, size_t lds, hipStream_t st) {
    return rt_launch_kernel(pick(spheres_only, tex_level, lds_mode), dim3(RT_AOV_THREADS), grid, lds, st, sd, ap, tp);
}

hipError_t rt_aov_through_occupancy(bool spheres_only, int tex_level, int lds_mode, size_t lds, int* blocks_per_cu) {
    return rt_kernel_occupancy(pick(spheres_only, tex_level, lds_mode), RT_AOV_THREADS, lds, blocks_per_cu);
}
