// rt_kernel_aov.hip -- rt_render_aov (include/rt_abi.h): the feature buffers of a frame -- albedo, normal, depth, coverage and
// the ids of the first hit -- from the primary rays rt_render would send.  Internal to librt_mi355x.so; launched by rt_abi.hip.
//
// One pixel per lane, persistent workgroups: each workgroup stages the scene into LDS once (stage_scene) and then strides
// over the frame's work items, 8 x 8 pixel tiles of 64 consecutive items as the render kernels cut them (work_to_pixel), so a
// wave's 64 primary rays leave through one compact block of the image plane and walk nearly the same nodes.  A lane keeps
// its whole pixel in registers -- the XORWOW state, the sample counter, the walk's state, the running sums -- and runs its
// samples as one state machine: every trip of the loop is one node visit for the lanes that are walking and, for the lanes
// whose walk has just ended, the hit record, the sample's terms and what follows (the next sample, or the stores and the
// lane's next pixel, taken at once).  No atomics, no inter-workgroup communication.
//
// The feature pass draws, per sample, what a render sample draws before its path (rt_kernel_pixel.hip: two jitter uniforms,
// camera_get_ray's lens-disk loop and its shutter uniform) and nothing else: sample s of a pixel is the primary ray rt_render
// would send if no path consumed a draw, sample 0 is rt_render's first primary ray of that pixel.
#include "rt_kernel_query.h"
#include "rt_launch.h"

namespace {

// the albedo of a hit (include/rt_abi.h): what a lambertian or isotropic surface attenuates by and what a light emits -- the
// texture's value at (u, v, p) or the inline colour, as shade() reads them --, a metal's colour, 1 for glass
template <int TEX>
DEV f3 hit_albedo(const SceneView& sc, const HitRec& rec) {
    const rt_material m = sc.materials[rec.mat];
    if (m.kind == RT_MAT_DIELECTRIC) return mk3(1.0f, 1.0f, 1.0f);
    if (TEX > 0 && m.kind != RT_MAT_METAL && m.tex >= 0) return texture_value<TEX>(sc, m.tex, rec.u, rec.v, rec.p);
    return ld3(m.albedo);
}

template <bool SPHERES_ONLY, int TEX, int LDS_MODE>
__global__ void __launch_bounds__(RT_AOV_THREADS) rt_aov_kernel(rt_scene_dev sd, rt_aov_params ap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const SceneView sc = stage_scene<LDS_MODE>(sd, lds);
    const float4* nodes4 = reinterpret_cast<const float4*>(sc.nodes);
    const int nn = sc.n_nodes;
    // work item w = (tile << 6) | position in the tile; the grid's stride is a multiple of 64, so a lane keeps its position and
    // a wave always holds one whole tile
    const uint32_t items = ap.work_items, stride = gridDim.x * blockDim.x;
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    // what the requested outputs need (grid-uniform): the hit record for normal, albedo and mat; the texture and its (u, v)
    // for albedo alone
    const bool want_albedo = ap.albedo != nullptr;
    const bool want_rec = want_albedo || ap.normal != nullptr || ap.mat != nullptr;

    rt_xorwow g;
    Ray cur;
    f3 inv;
    LooseRay lr;
    bool loose = false;
    HitInfo best;
    int node = nn, sample = 0, i = 0, j = 0;
    size_t px = 0;               // lrow * nx + i: the pixel's place in every output
    f3 alb, nrm;
    float depth = 0.0f, alpha = 0.0f;

    auto start_sample = [&]() {  // rt_kernel_pixel.hip: the sample's place in the pixel, then camera_get_ray's draws
        const float u = ((float)i + rt_xorwow_uniform(g)) / (float)ap.nx;
        const float v = ((float)j + rt_xorwow_uniform(g)) / (float)ap.ny;
        cur = camera_get_ray(sd.camera, u, v, g);
        walk_start(cur, sd.bound, FLT_MAX, best, inv, loose, lr, node);   // world->hit for `cur` (main.cu:57)
    };
    // the lane's next work item that is a pixel of the frame (tiles overhang its right and top edges); rt_kernel_aov_through.hip
    // has the same lambda
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
        depth = 0.0f; alpha = 0.0f;
        sample = 0;
        start_sample();
    };

    begin();
    while (__ballot(w < items) != 0ull) {
        if (node < nn) node = walk_step<SPHERES_ONLY, false>(sc, nodes4, node, cur, inv, lr, loose, 0.001f, best);   // main.cu:57
        if (w < items && node >= nn) {   // this sample's walk is over: its terms, summed in sample order
            const bool hit = best.prim >= 0;
            int32_t mat = -1;
            if (hit) {
                if (want_rec) {
                    // the sphere's (u, v) -- acos / atan2 in double -- only under a texture that reads it, and only for albedo
                    const HitRec rec = (TEX == 2 && want_albedo) ? resolve_hit<SPHERES_ONLY, true>(sc, cur, best)
                                                                 : resolve_hit<SPHERES_ONLY, false>(sc, cur, best);
                    nrm = nrm + rec.n;
                    mat = rec.mat;
                    if (want_albedo) alb = alb + hit_albedo<TEX>(sc, rec);
                }
                depth = depth + best.t;
                alpha = alpha + 1.0f;
            } else if (want_albedo) {
                alb = alb + miss_color(ap, cur);
            }
            if (sample == 0) {           // the ids are the first sample's (rt_trace_rays' prim_out / inst_out / mat_out)
                if (ap.prim) ap.prim[px] = best.prim;
                if (ap.inst) ap.inst[px] = best.inst;
                if (ap.mat) ap.mat[px] = mat;
            }
            if (++sample < ap.ns) {
                start_sample();
            } else {
                const float k = (float)(1.0 / (double)(float)ap.ns);   // store_pixel: vec3::operator/=(float), vec3.cuh:145-153
                if (want_albedo) st3(ap.albedo + 3 * px, alb, k);
                if (ap.normal) st3(ap.normal + 3 * px, nrm, k);
                if (ap.depth) ap.depth[px] = depth * k;
                if (ap.alpha) ap.alpha[px] = alpha * k;
                w += stride;
                begin();
            }
        }
    }
}

using Kernel = void (*)(rt_scene_dev, rt_aov_params);

template <bool SO, int TEX>
Kernel pick_lds(int lds_mode) {
    if (lds_mode == 2) return rt_aov_kernel<SO, TEX, 2>;
    if (lds_mode == 1) return rt_aov_kernel<SO, TEX, 1>;
    return rt_aov_kernel<SO, TEX, 0>;
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

hipError_t rt_launch_aov(bool spheres_only, int tex_level, int lds_mode, const rt_scene_dev& sd, const rt_aov_params& ap, dim3 grid,
                         size_t lds, hipStream_t st) {
    return rt_launch_kernel(pick(spheres_only, tex_level, lds_mode), dim3(RT_AOV_THREADS), grid, lds, st, sd, ap);
}

hipError_t rt_aov_occupancy(bool spheres_only, int tex_level, int lds_mode, size_t lds, int* blocks_per_cu) {
    return rt_kernel_occupancy(pick(spheres_only, tex_level, lds_mode), RT_AOV_THREADS, lds, blocks_per_cu);
}
