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
#include "rt_device_funcs.h"

namespace {

// One node visit of the walk for a ray with the window (0.001, best.t): twin of rt_kernel_radiance.hip's walk_step (and of
// trace_step<SPHERES_ONLY, false> in rt_kernel_trace.hip with tmin fixed): a change to one belongs in the others (kept apart
// so that those units compile to the assembly they had).  `loose`: interior boxes take the widened one-fma form and a leaf's
// own box is tested again exactly before its object; otherwise (a zero direction component) the reference's
// own slab form everywhere.  Returns the next node.
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

// the miss term of color() (main.cu:59-65): miss_color() for this pass's argument block
DEV f3 miss_term(const rt_aov_params& ap, const Ray& r) {
    f3 bg = mk3(ap.background[0], ap.background[1], ap.background[2]);
    if (ap.use_gradient_bg) {
        const f3 ud = unit_vector(r.d);
        const float t = 0.5f * (ud.y + 1.0f);
        bg = mk3(fmaf(t, 0.5f, 1.0f - t), fmaf(t, 0.7f, 1.0f - t), (1.0f - t) + t);
    }
    return bg;
}

// the albedo of a hit (include/rt_abi.h): what a lambertian or isotropic surface attenuates by and what a light emits -- the
// texture's value at (u, v, p) or the inline colour, as shade() reads them --, a metal's colour, 1 for glass
template <int TEX>
DEV f3 hit_albedo(const SceneView& sc, const HitRec& rec) {
    const rt_material m = sc.materials[rec.mat];
    if (m.kind == RT_MAT_DIELECTRIC) return mk3(1.0f, 1.0f, 1.0f);
    if (TEX > 0 && m.kind != RT_MAT_METAL && m.tex >= 0) return texture_value<TEX>(sc, m.tex, rec.u, rec.v, rec.p);
    return ld3(m.albedo);
}

DEV void st3(float* p, f3 v, float k) { p[0] = v.x * k; p[1] = v.y * k; p[2] = v.z * k; }

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
        best.t = FLT_MAX; best.prim = -1; best.inst = -1;   // world->hit for `cur` (main.cu:57)
        inv = mk3(1.0f / cur.d.x, 1.0f / cur.d.y, 1.0f / cur.d.z);
        loose = inv_is_finite(inv) && loose_ok(inv, cur.o, sd.bound);
        lr = loose_setup(inv, cur.o, sd.bound);
        node = 0;
    };
    // the lane's next work item that is a pixel of the frame (tiles overhang its right and top edges)
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
        if (node < nn) node = walk_step<SPHERES_ONLY>(sc, nodes4, node, cur, inv, lr, loose, best);
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
                alb = alb + miss_term(ap, cur);
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

template <bool SO, int TEX, int LM>
hipError_t set_lds(size_t lds) {
    if (lds <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&rt_aov_kernel<SO, TEX, LM>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

template <bool SO, int TEX, int LM>
struct Launch {
    static hipError_t run(const rt_scene_dev* sd, const rt_aov_params* ap, dim3 grid, size_t lds, hipStream_t st) {
        const hipError_t e = set_lds<SO, TEX, LM>(lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((rt_aov_kernel<SO, TEX, LM>), grid, dim3(RT_AOV_THREADS), lds, st, *sd, *ap);
        return hipGetLastError();
    }
};
template <bool SO, int TEX, int LM>
struct Occupancy {
    static hipError_t run(size_t lds, int* blocks) {
        const hipError_t e = set_lds<SO, TEX, LM>(lds);
        if (e != hipSuccess) return e;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void*>(&rt_aov_kernel<SO, TEX, LM>),
                                                            RT_AOV_THREADS, lds);
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

hipError_t rt_launch_aov(bool spheres_only, int tex_level, int lds_mode, const rt_scene_dev& sd, const rt_aov_params& ap, dim3 grid,
                         size_t lds, hipStream_t st) {
    return dispatch<Launch>(spheres_only, tex_level, lds_mode, &sd, &ap, grid, lds, st);
}

hipError_t rt_aov_occupancy(bool spheres_only, int tex_level, int lds_mode, size_t lds, int* blocks_per_cu) {
    return dispatch<Occupancy>(spheres_only, tex_level, lds_mode, lds, blocks_per_cu);
}
