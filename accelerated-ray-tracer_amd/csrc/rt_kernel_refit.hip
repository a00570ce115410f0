// rt_kernel_refit.hip -- the device half of rt_scene_update_spheres, rt_scene_update_instances and rt_scene_update_quads
// (include/rt_abi.h): spheres, instances or quads of a resident scene are replaced and every box that
// depends on them is recomputed where it lives, with the topology of every array kept.
//
// One path for the three kinds: launches on one stream, each complete before the next starts (that order is the only
// synchronisation there is):
//   1. records   one lane per record: check it (device-resident records reach no host check), store it, stamp the record it
//                replaces.  A kernel per kind: they differ in what they check and in what they store beside the record;
//   1b. marks    quads only, one lane per box: the data rt_scene_create derives from quad records (the axis code in pad0, which
//                the records kernel stores, and the canonical mark in bit 30 of first_quad) follow the records;
//   2. leaves    one lane per leaf: a leaf whose solid depends on a record with this update's stamp (rt_refit::depends_on) takes
//                its rule's box (rt_refit::solid_box), written to the canonical leaf arrays, the tier arrays (xyz only) and the
//                leaf's node in both node arrays.  One kernel, instantiated per kind;
//   3. slots     one wave per 64 leaves: the union of their boxes and their largest |coordinate|, by cross-lane min / max;
//   4. interior  one wave per interior node of either array: the union over its leaf range [a, b) as partial head leaves, whole
//                slots from step 3 and partial tail leaves -- at most 126 + (b - a) / 64 reads whatever the tree's shape --;
//                one further wave reduces the slots' largest coordinates to the scene's bound.
// Steps 3 and 4 do not care why a leaf's box changed.
// Float min / max are exact, so no result depends on the order of a reduction (up to the sign of a zero).  No address depends
// on record data: every index comes from the host's tables or from the index list the host has checked.
// The render kernels read some of these arrays through the scalar cache (uniform_load, rt_device_funcs.h); that stays correct
// because none of them runs concurrently with these launches and the cache does not outlive a dispatch.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "rt_device.h"
#include "rt_refit_host.h"

namespace {

__device__ inline float wave_min(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

struct box6 { float lo[3], hi[3]; };
__device__ inline box6 empty_box() { return {{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}}; }
__device__ inline void grow(box6& b, const float4 lo, const float4 hi) {
    b.lo[0] = fminf(b.lo[0], lo.x); b.lo[1] = fminf(b.lo[1], lo.y); b.lo[2] = fminf(b.lo[2], lo.z);
    b.hi[0] = fmaxf(b.hi[0], hi.x); b.hi[1] = fmaxf(b.hi[1], hi.y); b.hi[2] = fmaxf(b.hi[2], hi.z);
}
__device__ inline void wave_union(box6& b) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { b.lo[c] = wave_min(b.lo[c]); b.hi[c] = wave_max(b.hi[c]); }
}

__global__ __launch_bounds__(RT_REFIT_THREADS) void rt_refit_records_kernel(const rt_refit_params p) {
    const int k = (int)(blockIdx.x * RT_REFIT_THREADS + threadIdx.x);
    if (k >= p.count) return;
    const rt_sphere rec = static_cast<const rt_sphere*>(p.records)[k];
    if (!rt_refit::record_ok(rec, p.n_materials)) {
        atomicOr(reinterpret_cast<unsigned int*>(p.result) + 3, 1u);    // refused: the sphere, its stamp and its boxes stay
        return;
    }
    const int i = p.indices ? p.indices[k] : p.first + k;                 // checked on the host: in range, each at most once
    p.spheres[i] = rec;
    p.stamp[i] = p.epoch;
}

// leaf q's new box, everywhere it lives: the canonical arrays, the tier arrays (xyz only) and the leaf's node in both node arrays
__device__ inline void store_leaf(const rt_refit_params& p, int q, const float lo[3], const float hi[3]) {
    p.box_lo[q] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    p.box_hi[q] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    if (p.tier_lo) {
        float* tl = reinterpret_cast<float*>(p.tier_lo + q);
        float* th = reinterpret_cast<float*>(p.tier_hi + q);
        for (int c = 0; c < 3; ++c) { tl[c] = lo[c]; th[c] = hi[c]; }
    }
    rt_node* n = p.nodes_ref + p.leaf_node_ref[q];
    for (int c = 0; c < 3; ++c) { n->bmin[c] = lo[c]; n->bmax[c] = hi[c]; }
    if (p.nodes_walk) {
        n = p.nodes_walk + p.leaf_node_walk[q];
        for (int c = 0; c < 3; ++c) { n->bmin[c] = lo[c]; n->bmax[c] = hi[c]; }
    }
}

// One lane per leaf: a leaf whose solid depends on a record of KIND with this update's stamp takes its rule's box from the records
// where they live (a sphere, a quad, the six quads of a box, or the instance rule over one of these).  Addresses: leaf_solid (the
// host's table), the stored instance child, first_quad with its marks masked.
template <int KIND>
__global__ __launch_bounds__(RT_REFIT_THREADS) void rt_refit_leaves_kernel(const rt_refit_params p) {
    const int q = (int)(blockIdx.x * RT_REFIT_THREADS + threadIdx.x);
    if (q >= p.n_leaves) return;
    const int32_t solid = p.leaf_solid[q];
    const uint32_t* stamp = p.stamp;
    const uint32_t epoch = p.epoch;
    if (!rt_refit::depends_on(KIND, solid, p.boxes, p.instances, [=](int i) { return stamp[i] == epoch; })) return;
    float lo[3], hi[3];
    rt_refit::solid_box(solid, p.spheres, p.quads, p.boxes, p.instances, lo, hi);
    store_leaf(p, q, lo, hi);
}

// An instance record is stored when it passes the checks and names the child the scene holds for that instance, so the stored
// child never changes: it stays the reference rt_scene_create validated, and the leaf kernel forms addresses from nothing else.
__global__ __launch_bounds__(RT_REFIT_THREADS) void rt_refit_instance_records_kernel(const rt_refit_params p) {
    const int k = (int)(blockIdx.x * RT_REFIT_THREADS + threadIdx.x);
    if (k >= p.count) return;
    const int i = p.indices ? p.indices[k] : p.first + k;                 // checked on the host: in range, each at most once
    const rt_instance rec = static_cast<const rt_instance*>(p.records)[k];
    if (!rt_refit::instance_record_ok(rec, p.instances[i].child)) {
        atomicOr(reinterpret_cast<unsigned int*>(p.result) + 3, 1u);    // refused: the instance, its stamp and its boxes stay
        return;
    }
    p.instances[i] = rec;
    p.stamp[i] = p.epoch;
}

// ---- rt_scene_update_quads
// One lane per record: the checks, the axis code rt_scene_create would have derived (the same function), the store, the stamp.
__global__ __launch_bounds__(RT_REFIT_THREADS) void rt_refit_quad_records_kernel(const rt_refit_params p) {
    const int k = (int)(blockIdx.x * RT_REFIT_THREADS + threadIdx.x);
    if (k >= p.count) return;
    rt_quad rec = static_cast<const rt_quad*>(p.records)[k];
    if (!rt_refit::quad_record_ok(rec, p.n_materials)) {
        atomicOr(reinterpret_cast<unsigned int*>(p.result) + 3, 1u);    // refused: the quad, its stamp, its boxes and marks stay
        return;
    }
    const int i = p.indices ? p.indices[k] : p.first + k;                 // checked on the host: in range, each at most once
    rec.pad0 = __int_as_float(rt_refit::axis_code(rec));
    p.quads[i] = rec;
    p.stamp[i] = p.epoch;
}

// One lane per box, after every record is stored (a launch of its own: box ranges may overlap, and a lane that stores one face
// cannot know whether another has been stored): bit 30 of first_quad from the six faces' codes.  Nothing else of the word changes.
__global__ __launch_bounds__(RT_REFIT_THREADS) void rt_refit_box_marks_kernel(const rt_refit_params p) {
    const int b = (int)(blockIdx.x * RT_REFIT_THREADS + threadIdx.x);
    if (b >= p.n_boxes) return;
    const int32_t word = p.boxes[b].first_quad, first = word & RT_BOX_FIRST_MASK;
    int32_t codes[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) codes[f] = __float_as_int(p.quads[first + f].pad0);
    const int32_t marked = rt_refit::canonical_codes(codes) ? (word | RT_BOX_CANONICAL) : (word & ~RT_BOX_CANONICAL);
    if (marked != word) p.boxes[b].first_quad = marked;
}

__global__ __launch_bounds__(RT_REFIT_THREADS) void rt_refit_slots_kernel(const rt_refit_params p) {
    const int k = (int)(blockIdx.x * (RT_REFIT_THREADS / 64) + threadIdx.x / 64), lane = (int)(threadIdx.x & 63);
    if (k >= p.n_slots) return;                                         // (whole waves leave together)
    const int q = k * 64 + lane;
    box6 b = empty_box();
    float ab[3] = {0.0f, 0.0f, 0.0f};
    if (q < p.n_leaves) {                                               // padding leaves take part in nothing
        const float4 lo = p.box_lo[q], hi = p.box_hi[q];
        grow(b, lo, hi);
        ab[0] = fmaxf(fabsf(lo.x), fabsf(hi.x)); ab[1] = fmaxf(fabsf(lo.y), fabsf(hi.y)); ab[2] = fmaxf(fabsf(lo.z), fabsf(hi.z));
    }
    wave_union(b);
#pragma unroll
    for (int c = 0; c < 3; ++c) ab[c] = wave_max(ab[c]);
    if (lane == 0) {
        float* r = p.slot_box + (size_t)k * 8;
        for (int c = 0; c < 3; ++c) { r[c] = b.lo[c]; r[3 + c] = b.hi[c]; p.slot_abs[(size_t)k * 4 + c] = ab[c]; }
    }
}

__global__ __launch_bounds__(RT_REFIT_THREADS) void rt_refit_interior_kernel(const rt_refit_params p) {
    const int w = (int)(blockIdx.x * (RT_REFIT_THREADS / 64) + threadIdx.x / 64), lane = (int)(threadIdx.x & 63);
    if (w > p.n_jobs) return;
    if (w == p.n_jobs) {                                                // the bound: the largest |coordinate| of any leaf, per axis
        float ab[3] = {0.0f, 0.0f, 0.0f};
        for (int k = lane; k < p.n_slots; k += 64)
            for (int c = 0; c < 3; ++c) ab[c] = fmaxf(ab[c], p.slot_abs[(size_t)k * 4 + c]);
#pragma unroll
        for (int c = 0; c < 3; ++c) ab[c] = wave_max(ab[c]);
        if (lane == 0) for (int c = 0; c < 3; ++c) p.result[c] = ab[c];
        return;
    }
    const int4 job = p.jobs[w];
    const int a = job.y, e = job.z;
    if (e <= a) return;                                                 // an interior node over no leaf keeps its box
    box6 b = empty_box();
    const int s0 = (a + 63) >> 6, s1 = e >> 6;                          // whole slots [s0, s1)
    if (s0 >= s1) {                                                     // no whole slot: fewer than 128 leaves
        for (int q = a + lane; q < e; q += 64) grow(b, p.box_lo[q], p.box_hi[q]);
    } else {
        int q = a + lane;
        if (q < s0 * 64) grow(b, p.box_lo[q], p.box_hi[q]);             // head: fewer than 64 leaves
        for (int k = s0 + lane; k < s1; k += 64) {
            const float* r = p.slot_box + (size_t)k * 8;
            grow(b, make_float4(r[0], r[1], r[2], 0.0f), make_float4(r[3], r[4], r[5], 0.0f));
        }
        q = s1 * 64 + lane;
        if (q < e) grow(b, p.box_lo[q], p.box_hi[q]);                   // tail: fewer than 64 leaves
    }
    wave_union(b);
    if (lane == 0) {
        rt_node* n = (job.w ? p.nodes_walk : p.nodes_ref) + job.x;
        for (int c = 0; c < 3; ++c) { n->bmin[c] = b.lo[c]; n->bmax[c] = b.hi[c]; }
    }
}

inline unsigned int blocks_for(long long items, int per_block) { return (unsigned int)((items + per_block - 1) / per_block); }

}  // namespace

hipError_t rt_launch_refit(const rt_refit_params& p, int kind, hipStream_t st) {
    const dim3 threads(RT_REFIT_THREADS);
    const auto records = kind == rt_refit::QUADS ? rt_refit_quad_records_kernel : kind == rt_refit::INSTANCES ? rt_refit_instance_records_kernel : rt_refit_records_kernel;
    const auto leaves = kind == rt_refit::QUADS ? rt_refit_leaves_kernel<rt_refit::QUADS>
                        : kind == rt_refit::INSTANCES ? rt_refit_leaves_kernel<rt_refit::INSTANCES> : rt_refit_leaves_kernel<rt_refit::SPHERES>;
    if (p.count > 0) hipLaunchKernelGGL(records, dim3(blocks_for(p.count, RT_REFIT_THREADS)), threads, 0, st, p);
    if (kind == rt_refit::QUADS && p.count > 0 && p.n_boxes > 0)
        hipLaunchKernelGGL(rt_refit_box_marks_kernel, dim3(blocks_for(p.n_boxes, RT_REFIT_THREADS)), threads, 0, st, p);
    if (p.count > 0 && p.n_leaves > 0) hipLaunchKernelGGL(leaves, dim3(blocks_for(p.n_leaves, RT_REFIT_THREADS)), threads, 0, st, p);
    const int waves = RT_REFIT_THREADS / 64;                            // steps 3 and 4
    if (p.n_slots > 0) hipLaunchKernelGGL(rt_refit_slots_kernel, dim3(blocks_for(p.n_slots, waves)), threads, 0, st, p);
    hipLaunchKernelGGL(rt_refit_interior_kernel, dim3(blocks_for((long long)p.n_jobs + 1, waves)), threads, 0, st, p);
    return hipGetLastError();
}
