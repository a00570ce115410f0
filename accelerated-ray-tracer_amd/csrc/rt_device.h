// rt_device.h -- kernel argument blocks shared by the kernel translation units (rt_kernel_pixel.hip, rt_staged_*.hip,
// rt_tier_*.hip, rt_rank.hip) and the host units (rt_abi.hip, rt_abi_debug.hip: the C-ABI implementation).  Internal to librt_mi355x.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_abi.h"

#define RT_PERSISTENT_THREADS 512   // default workgroup size of the staged kernel
// Register budgets of the staged kernel families, as launch bounds (threads per workgroup the code may be launched
// with, waves per SIMD it must leave room for).  "Lean" = spheres-only scenes without procedural / image textures (the
// headline kernel): 101 VGPRs (allocated in eights: 104), no scratch (profiles/r03_kernel_resources.md) -- the double-precision
// transcendentals are out of line and the one-pixel-per-wave loops live in their own kernel (rt_kernel_tier.h).  It is launched
// 2 x 512 threads per CU = 4 waves per SIMD: 4 x 104 registers leave 96 of a SIMD's 512 for one co-resident wave of the tier
// kernel (78, allocated 80).  104 is therefore this kernel's ceiling, not the 128 the launch bounds would allow.
// Everything else (quads / boxes / media, Perlin / image textures) is budgeted 168 VGPRs: 3 waves per SIMD.
#ifndef RT_LEAN_MIN_WAVES
#define RT_LEAN_MIN_WAVES 4
#endif
#ifndef RT_LEAN_MAX_THREADS
#define RT_LEAN_MAX_THREADS 512
#endif
#define RT_HEAVY_MAX_THREADS 768
#define RT_HEAVY_MIN_WAVES 3

// the tier kernel (rt_kernel_tier.h): workgroups of four waves, one per SIMD; the lean family's must fit beside the main kernel's
// 4 x 104 registers per SIMD (they take 76), the others get 168 (their workgroups take the slots main workgroups vacate: main_skip_wgs)
#define RT_TIER_THREADS 256
// kernel ids keep their round-1 numbers (1 = persistent, 2 = parked, 4 = wavefront were experiments; removed)
// the statistics block behind rt_frame_params.ray_counter (64-bit words): [0] rays, [1..16] stage counters and [32..] the
// wave-end histograms of diagnostic builds (-DRT_DIAG), [3] the sum of the cost prior (rt_prior_kernel)
enum { RT_DIAG_BINS = 192, RT_DIAG_T0_SLOT = 32, RT_DIAG_HIST_SLOT = 33, RT_DIAG_WAVE_SLOT = 33 + 2 * 192 + 7, RT_DIAG_MAX_WAVES = 8192,
       RT_COUNTER_BYTES = (33 + 2 * 192 + 7 + 2 * 8192) * 8 };   // + per wave: two words about the lane that finished last
enum { RT_KERNEL_PIXEL = 0, RT_KERNEL_STAGED = 3 };

// A pixel parked at a sample boundary (split frames): XORWOW state, colour sum, rays traced so far.
struct rt_pixel_state {
    uint32_t rng[6];
    float col[3];
    uint32_t cost;               // rays so far; bit 31 = "on the heavy list of the coming launch" (set by the ranking)
};

// What the ranking kernels (rt_rank.hip) leave for the next render launch of a split frame: how many parked pixels are
// "heavy", how the heavy list is cut into tiers and how many workgroups serve each.  Lives in device memory; the render
// kernel reads it at its start, the host never does (a frame is one stream enqueue, no round trip).
struct rt_rank_info {
    uint32_t heavy_items;        // entries of heavy_pixels (dearest first); 0 = no list
    uint32_t heavy_threshold;    // pixels whose parked cost is >= this are in the list (ordinary waves skip them)
    uint32_t tier1_items;        // leading entries served one per WAVE by the tier kernel (tier 1)
    uint32_t tier2_items;        // following entries served by sparse waves (tier 2); the REST of the list (tier 3) is taken by
                                 // ordinary lanes before anything else, so that every dear pixel's chain starts at once
    int32_t tier1_wgs;           // workgroups of the TIER kernel that have work (the rest of its grid leaves at once)
    int32_t main_skip_wgs;       // workgroups [0, main_skip_wgs) of the MAIN kernel leave at once: their slots are the tier
                                 // kernel's (kernel families whose register budget leaves no room beside a full main grid)
    int32_t sparse_wgs;          // main workgroups [main_skip_wgs, main_skip_wgs + sparse_wgs) start in sparse mode (tier 2)
    int32_t sparse_stride;       // sparse waves: every sparse_stride-th lane takes a pixel
    int32_t semi_wgs;            // the next semi_wgs workgroups serve tier 3 with every semi_stride-th lane (0: ordinary lanes take tier 3)
    int32_t semi_stride;
    uint32_t threshold1;         // cost that qualifies for tier 1 (set with heavy_threshold by the first ranking kernel)
    uint32_t threshold2;         // cost that qualifies for the sparse waves (tier 2)
    uint32_t collected;          // entries rt_collect_heavy_kernel appended (may exceed the capacity: then there is no list)
};

// constants of one ranking (host-filled kernel argument)
struct rt_rank_params {
    rt_pixel_state* state;               // (the ranking marks listed pixels in bit 31 of their cost)
    const unsigned int* tile_cost;
    unsigned int* tile_order;
    const unsigned long long* ray_counter;
    unsigned long long* heavy_list;      // scratch: (cost << 32 | pixel), unsorted
    unsigned int* heavy_pixels;          // out: pixel ids, dearest first
    rt_rank_info* info;
    uint32_t n_pixels, n_tiles, heavy_cap;
    uint32_t max_grid, waves_per_wg, normal_need;
    int32_t sparse_stride;               // 0 = no heavy list at all
    int32_t semi_stride;                 // lanes per pixel in the workgroups that serve tier 3 (0 = ordinary lanes take tier 3 first)
    int32_t sparse_percent;              // at most this share of max_grid starts in sparse mode
    int32_t sparse_work_percent;         // ... and tiers 0-2 together hold at most this share of the frame's rays so far
    int32_t tier_possible;               // the scene has tier data (leaf arrays, rt_scene_dev) and the tier kernel is launched
    int32_t tier1_pixels;                // cap on tier 1
    int32_t tier1_depth;                 // pixels a tier-1 wave is meant to take, one after the other
    int32_t tier_wgs_cap;                // the tier kernel's grid (fixed on the host before the sizes are known)
    int32_t tier_waves_per_main_wg;      // 0: tier workgroups fit beside a full main grid; else: tier waves that fit into the
                                         // slot of one main workgroup (main_skip_wgs = tier waves / this, rounded up)
    int32_t nx, smooth_percent;          // cost estimate of a pixel = max(own, smooth_percent % of its dearest 4-neighbour's); nx = pixels per local row
    float heavy_factor, sparse_factor, tier1_factor;   // cost thresholds as multiples of the mean cost per pixel:
                                         // >= heavy: in the list at all; >= sparse: tier 2; >= tier1: tier 1
};

// Device encoding of a node's two links (both node arrays below; rt_abi.hip device_nodes()): `skip` holds ~skip and
// `prim` holds ~(own index + 1) at an interior node (still < 0) and the object id (>= 0) at a leaf.  The walk's "where
// next" is then ~((pass && prim < 0) ? prim : skip) -- one select, one NOT -- and the staged kernel's stopped state
// ~skip is the stored word itself.
// The main kernel's LDS image differs from these arrays: with its nodes in LDS (lds_mode 1-3) it walks LDS addresses, and
// while it stages the array it rewrites the two words for that walk (stage_scene<.., true>, rt_device_funcs.h) -- skip =
// LDS address of the skip target, prim = LDS address of the next record at an interior node and ~(the record's own LDS
// address) (< 0) at a leaf, whose object reference moves to a word table behind the image (4 bytes a record, padded to 16:
// RT_WALK_PRIM_TABLE_BYTES, part of the launch's LDS size).  "Where next" is then (pass && (inner || a leaf is noted)) ?
// prim : skip -- one select, no NOT, no address arithmetic before the reads -- and a lane stopped at a leaf holds that
// leaf's address in its state.  Nothing outside that kernel sees the image: the device arrays, every other kernel, the
// refit kernels and rt_debug_scene_boxes keep the encoding above, as does the main kernel with lds_mode 0 and 4.
#define RT_NODE_SKIP(stored) (~(stored))
#define RT_WALK_PRIM_TABLE_BYTES(n_nodes) ((4 * (n_nodes) + 15) & ~15)

// device-resident scene: the rt_scene_desc arrays after upload
struct rt_scene_dev {
    const rt_node* nodes;        // the walk array: the reference's tree in depth-first order, interior nodes that do not pay removed (rt_abi.hip, "collapse")
    const rt_node* nodes_ref;    // the reference's tree, every node (kernel 0 and the calibration pass walk this one)
    const rt_sphere* spheres;
    const rt_quad* quads;
    const rt_box* boxes;
    const rt_instance* instances;
    const rt_medium* media;
    const rt_material* materials;
    const rt_texture* textures;
    const uint8_t* images;
    int32_t n_nodes, n_nodes_ref, n_spheres, n_materials, n_textures;
    float bound[3];              // every box coordinate of the scene lies within +-bound[axis] (the walk loop's widened box test)
    float bound_pad;
    // tier data (rt_kernel_tier.h; built by rt_scene_create from the walk array, null when the scene has none): the leaves
    // of the walk array in depth-first order as two float4 arrays padded to a multiple of 64 -- leaf_lo[q] = (bmin, prim as
    // int bits; -1 in the padding), leaf_hi[q] = (bmax, 0) --, per 64 leaves the union of their boxes (slot_ranges: 8 floats
    // each: lo, hi, 0, 0), and the ordinals of the (at most two) constant_medium leaves
    const float4* leaf_lo;
    const float4* leaf_hi;
    const float* slot_ranges;
    int32_t n_leaves, n_slots;
    int32_t n_media_leaves;
    int32_t media_ord[2];
    rt_camera camera;
};

enum { RT_WC_DEAD = 64,        // work_counter[]: lanes of the main launch that have run out of work
       RT_WC_PUSHED = 65,      // entries pushed to handoff_queue
       RT_WC_TAIL_HEAD = 66,   // the tail launch's queue head
       RT_WORK_COUNTER_BYTES = 512 };
struct rt_frame_params {
    float* fb;                            // compact local rows, nx*3 floats each
    unsigned long long* ray_counter;      // += rays traced
    unsigned int* work_counter;           // persistent kernel's pixel queue head
    unsigned int* pixel_cost;             // calibration pass (kernel 0 only): rays traced per pixel, nx * local_rows; null otherwise
    unsigned int* node_pass;              // calibration pass (kernel 0 only): += 1 per box test of nodes_ref[i] that passed; null otherwise
    int32_t node_pass_lds;                // ... collected in LDS per workgroup (n_nodes_ref x 4 B of dynamic LDS) and flushed at its end
    float* ray_sample;                    // calibration pass: every ray_sample_stride-th ray as (origin, direction, t of its hit or FLT_MAX), 7 floats each
    uint32_t ray_sample_cap, ray_sample_stride;   // ... up to this many; the count is kept in ray_counter[2]
    const unsigned int* tile_order;       // optional: 8x8 tiles in descending cost (LPT order); null = natural order
    unsigned int* tile_cost;              // first part of a split frame: rays per 8x8 tile
    rt_pixel_state* state_out;            // first part of a split frame: where pixels are parked (the frame is not written)
    const rt_pixel_state* state_in;       // second part: the parked pixels (null = pixels start from their seed)
    int32_t sample_begin, sample_end;     // samples [sample_begin, sample_end) are rendered by this launch; ns is the frame's total
    const unsigned int* heavy_pixels;     // ranked launches: local pixel ids (lrow * nx + i) of the heavy pixels, dearest first
    const rt_rank_info* rank;             // ranked launches: tier sizes left by the ranking kernels; null = no heavy list, no tiers
    int32_t store_parked;                 // progressive windows (rt_render_window): a pixel parked at the window's end is ALSO written to fb,
                                          // averaged over the fp.ns samples so far
    int32_t fresh;                        // ranked FIRST part (tiers from the cost prior): state_in only carries the prior's cost and
                                          // list flag; pixels start from their seed with an empty colour sum
    int32_t tier_lds_scene;               // tier kernel: its LDS image holds spheres, materials and textures besides the leaf arrays
    // Tail hand-off (rt_abi.hip, "tail"): once the tile queue is dry and at most handoff_pixels pixels are still in flight on the
    // main kernel's lanes (= lanes that still have work), every lane parks its pixel at its next sample boundary into handoff_state[pixel] and pushes
    // (sample << 32 | pixel) to handoff_queue; the tier kernel, launched again AFTER the main kernel (tail_mode), finishes
    // them one pixel per wave.  Its counters live in a cache line of their own, away from the queue heads at work_counter[0..4]: with
    // the polled word in the queue heads' line every pixel fetch of the frame slowed down (headline 96 -> 118 ms).
    unsigned long long* handoff_queue;    // null = no hand-off
    uint32_t handoff_cap;                 // its entries
    rt_pixel_state* handoff_state;
    int32_t handoff_pixels;
    int32_t handoff_poll_ticks;           // ... looked for this often (10 ns ticks of s_memrealtime)
    int32_t tail_mode;                    // tier kernel: serve handoff_queue instead of tier 1 of the heavy list
    unsigned int* cost_out;               // last part of a ranked frame: every launch that writes a pixel's colour also writes the rays of its samples
                                          // [0, ns) here, bit 31 clear (the scene's cost map, rt_abi.hip); null = not written
    uint64_t seed_base;
    int32_t nx, ny, ns;
    float gamma;
    float background[3];
    int32_t use_gradient_bg;
    int32_t tile_rows, tile_first, tile_stride;
    int32_t local_rows;                   // rows this call renders
    int32_t tiles_x;                      // 8x8 pixel tiles per local row band
    uint32_t work_items;                  // tiles_x * tiles_y * 64
    int32_t sparse_eager;                 // staged kernel: sparse waves run every stage as soon as one lane needs it
    int32_t sparse_priority;              // staged kernel: s_setprio level of sparse waves (0 = leave alone)
    int32_t tier_priority;                // tier kernel: s_setprio level of its waves
    int32_t semi_priority;                // staged kernel: s_setprio level of the waves serving tier 3 on workgroups of their own
    int32_t steps_per_trip;               // persistent kernel: node visits between ballots
    int32_t shade_threshold;              // persistent kernel: waiting lanes that trigger shading
    int32_t leaf_threshold;               // staged kernel: lanes with an object test due that trigger the leaf pass
    int32_t box_threshold, medium_threshold;   // staged kernel, general scenes: parked box/instance and medium lanes that trigger their leaf tests
    int32_t diel_threshold;               // staged kernel: dielectric hits that trigger their stage
    int32_t newpath_threshold;            // staged kernel: ended paths that trigger the new-path stage
};

// the three ranking kernels of one ranked part, enqueued on `st` (no host synchronisation)
hipError_t rt_launch_rank(const rt_rank_params& rp, hipStream_t st);
// the cost prior of a ranked first part (rt_rank.hip): d_state[p].cost and tile_cost from the calibration frame's per-pixel rays
struct rt_prior_params {
    rt_pixel_state* state;
    unsigned int* tile_cost;
    unsigned long long* total;            // += sum of the priors (what the ranking kernels read as "rays so far")
    const unsigned int* cal_cost;         // rays per calibration pixel, cal_nx x cal_ny, row 0 = bottom
    int32_t cal_nx, cal_ny;
    int32_t nx, ny, local_rows, tiles_x;
    int32_t tile_rows, tile_first, tile_stride;
};
hipError_t rt_launch_prior(const rt_prior_params& pp, hipStream_t st);
// the same from the scene's cost map (rt_abi.hip): `cal_cost` holds one word per local pixel of THIS frame geometry (cal_nx, cal_ny are not read)
hipError_t rt_launch_prior_map(const rt_prior_params& pp, hipStream_t st);
// rt_debug_box_tests (rt_kernel_boxtest.hip): n cases, one per thread; device pointers, flags[n][4]
struct rt_box_test_params {
    int32_t n;
    const float* bmin;
    const float* bmax;
    const float* origins;
    const float* directions;
    const float* tmin;
    const float* tmax;
    float bound[3];
    uint8_t* flags;
};
hipError_t rt_launch_box_tests(const rt_box_test_params& bp, hipStream_t st);
// rt_debug_arith_tests (rt_kernel_arithtest.hip): device pointers; the modes are include/rt_abi.h's RT_ARITH_*.  The two draw
// modes run words [0, n), RT_ARITH_WORDS_PER_THREAD a thread, and read no array; RT_ARITH_LOOSE runs one ray per thread
#define RT_ARITH_WORDS_PER_THREAD 256u
struct rt_arith_test_params {
    int32_t mode;
    long long n;
    const float* a;
    const float* b;
    float bound[3];
    uint8_t* path;                // [n], or null: RT_ARITH_LOOSE's finite_inv per ray
    unsigned long long* out;      // [3], zeroed / ~0 / zeroed by the caller: mismatching cases, the first of them, rays with finite_inv
};
hipError_t rt_launch_arith_tests(const rt_arith_test_params& ap, hipStream_t st);
// rt_debug_math_tests (rt_kernel_arithtest.hip): device pointers; form and fn are include/rt_abi.h's RT_MATH_*.  The sweep runs
// words first .. first + count - 1, one workgroup per RT_MATH_WORDS_PER_GROUP of them, and adds into digests (zeroed by the caller);
// the list runs one element per thread
#define RT_MATH_WORDS_PER_GROUP (1u << 14)
struct rt_math_test_params {
    int32_t form, fn;
    uint32_t first;
    long long count;
    float operand;
    const float* a;
    const float* b;               // null where fn reads no second operand
    const float* c;               // null where fn reads no third operand
    float* out;                   // [count], RT_MATH_LIST
    unsigned long long* digests;  // [(count + 2^20 - 1) >> 20], RT_MATH_SWEEP
};
hipError_t rt_launch_math_tests(const rt_math_test_params& mp, hipStream_t st);
// bytes of the tier kernel's LDS image (rt_kernel_tier.h stages exactly this): leaf arrays + slot unions, then -- where the
// launch plan (rt_abi.hip) says so -- spheres, materials and textures
static inline size_t rt_tier_lds_bytes(int n_slots, int n_spheres, int n_materials, int n_textures, bool scene) {
    size_t b = (size_t)n_slots * 64 * 32 + (size_t)n_slots * 32;
    if (scene) b += (size_t)n_spheres * sizeof(rt_sphere) + (size_t)n_materials * sizeof(rt_material) + (size_t)n_textures * sizeof(rt_texture);
    return b;
}

// Launchers, one per translation unit (each returns the launch's hipError_t, including a failed
// hipFuncSetAttribute(MaxDynamicSharedMemorySize)).  tex_level: 0 = every material colour is inline, 1 = solid +
// checker textures, 2 = noise / image / noodle / felt / uv-offset textures too (Perlin noise and the sphere-uv
// transcendentals cost ~100 VGPRs, so scenes without them -- the headline random scene -- get leaner code).
hipError_t rt_launch_pixel(bool spheres_only, int tex_level, bool need_uv, const rt_scene_dev& sd, const rt_frame_params& fp,
                           dim3 grid, dim3 block, hipStream_t stream);
hipError_t rt_launch_staged_spheres(int tex_level, int lds_mode, const rt_scene_dev& sd, const rt_frame_params& fp, dim3 grid,
                                    dim3 block, size_t lds, hipStream_t st);
hipError_t rt_launch_staged_spheres_tex(int lds_mode, const rt_scene_dev& sd, const rt_frame_params& fp, dim3 grid, dim3 block,
                                        size_t lds, hipStream_t st);
hipError_t rt_launch_staged_general(int lds_mode, const rt_scene_dev& sd, const rt_frame_params& fp, dim3 grid, dim3 block,
                                    size_t lds, hipStream_t st);
hipError_t rt_launch_staged_general_tex(int lds_mode, const rt_scene_dev& sd, const rt_frame_params& fp, dim3 grid, dim3 block,
                                        size_t lds, hipStream_t st);
// the tier kernel of a ranked launch (rt_tier_*.hip); *vgprs_out (optional) = the instantiation's register count
hipError_t rt_launch_tier_spheres(int tex_level, const rt_scene_dev& sd, const rt_frame_params& fp, dim3 grid, size_t lds, hipStream_t st);
hipError_t rt_launch_tier_general(int tex_level, bool need_uv, const rt_scene_dev& sd, const rt_frame_params& fp, dim3 grid, size_t lds, hipStream_t st);

// rt_trace_rays (rt_kernel_trace.hip): one batch of caller rays, the pointers already checked on the host (rt_abi.hip)
struct rt_trace_params {
    int64_t n;
    const float* origins;
    const float* directions;
    const float* times;       // null = 0
    const float* tmax;        // null = FLT_MAX
    float tmin;
    int32_t record;           // some record output (point / normal / uv / mat) is requested
    float* t_out;
    int32_t* prim_out;
    int32_t* inst_out;
    float* point_out;
    float* normal_out;
    float* uv_out;
    int32_t* mat_out;
    uint8_t* hit_out;         // non-null: any-hit mode
};
// sd.nodes / sd.n_nodes: the node array to walk (the walk array or the reference's tree); lds_mode 0..2 as stage_scene;
// grid = persistent workgroups of RT_TRACE_THREADS.  rt_trace_occupancy: workgroups per CU of the instantiation a launch
// with these arguments would use, `lds` bytes of dynamic LDS each.
#define RT_TRACE_THREADS 256
hipError_t rt_launch_trace(bool spheres_only, int lds_mode, const rt_scene_dev& sd, const rt_trace_params& tp, dim3 grid, size_t lds,
                           hipStream_t st);
hipError_t rt_trace_occupancy(bool spheres_only, int lds_mode, bool any, bool record, size_t lds, int* blocks_per_cu);

// rt_radiance_rays (rt_kernel_radiance.hip): one batch of caller rays to shade, the pointers already checked on the host
struct rt_radiance_params {
    int64_t n;
    const float* origins;
    const float* directions;
    const float* times;       // null = 0
    const uint64_t* seeds;    // null = seed_base + i
    uint64_t seed_base;
    int32_t ns;
    int32_t use_gradient_bg;
    float background[3];
    float* rgb_out;
    uint32_t* rays_out;       // null = not written
};
// sd.nodes / sd.n_nodes: the walk array; tex_level as rt_launch_pixel; lds_mode 0..2 as stage_scene; grid = persistent
// workgroups of RT_RADIANCE_THREADS.  rt_radiance_occupancy: workgroups per CU of the instantiation such a launch would use.
#define RT_RADIANCE_THREADS 256
hipError_t rt_launch_radiance(bool spheres_only, int tex_level, int lds_mode, const rt_scene_dev& sd, const rt_radiance_params& rp,
                              dim3 grid, size_t lds, hipStream_t st);
hipError_t rt_radiance_occupancy(bool spheres_only, int tex_level, int lds_mode, size_t lds, int* blocks_per_cu);

// rt_render_aov (rt_kernel_aov.hip): the feature pass of one frame, the pointers already checked on the host.  Every output is
// optional (null = not written) and holds compact local rows like rt_frame_params.fb.
struct rt_aov_params {
    float* albedo;            // local_rows * nx * 3
    float* normal;            // local_rows * nx * 3
    float* depth;             // local_rows * nx
    float* alpha;             // local_rows * nx
    int32_t* prim;            // local_rows * nx each: the first sample's ids
    int32_t* inst;
    int32_t* mat;
    uint64_t seed_base;
    int32_t nx, ny, ns;
    int32_t use_gradient_bg;
    float background[3];
    int32_t tile_rows, tile_first, tile_stride;
    int32_t local_rows;       // rows this call renders
    int32_t tiles_x;          // 8x8 pixel tiles per local row band
    uint32_t work_items;      // tiles_x * tiles_y * 64, as rt_frame_params
};
// sd.nodes / sd.n_nodes: the walk array; tex_level as rt_launch_pixel; lds_mode 0..2 as stage_scene; grid = persistent
// workgroups of RT_AOV_THREADS.  rt_aov_occupancy: workgroups per CU of the instantiation such a launch would use.
#define RT_AOV_THREADS 256
hipError_t rt_launch_aov(bool spheres_only, int tex_level, int lds_mode, const rt_scene_dev& sd, const rt_aov_params& ap, dim3 grid,
                         size_t lds, hipStream_t st);
hipError_t rt_aov_occupancy(bool spheres_only, int tex_level, int lds_mode, size_t lds, int* blocks_per_cu);

// rt_denoise (rt_kernel_denoise.hip): the pack pass and one iteration of the filter, the pointers already checked on the host.
// A pixel is two 16-byte records in the workspace: colour (x.rgb, (x.r + x.g) + x.b) and guide (N.xyz, Z; zeros where absent).
struct rt_denoise_params {
    const float* color;       // pack: the planar inputs (albedo, normal, depth may be null)
    const float* albedo;      // ... and, when `demodulate`, read again by the last iteration
    const float* normal;
    const float* depth;
    float* out;               // last iteration: ny * nx * 3
    const float4* x_in;       // iteration: x_k
    float4* x_out;            // pack: x_0; iteration (not the last): x_{k+1}
    float4* guide;            // pack writes, iterations read; unused when no guide factor is on
    int32_t nx, ny;
    int32_t tiles_x;          // 16x16-pixel workgroup tiles per row band
    int32_t step;             // s = 2^k
    int32_t normal_sharpness; // m
    int32_t demodulate;
    int32_t last;
    float sigma_color_k;      // sigma_color * 2^-k
    float color_floor;
    float sigma_depth;
};
#define RT_DENOISE_THREADS 256
#define RT_DENOISE_TILE 16
#define RT_DENOISE_MAX_STAGED_STEP 8
// the LDS image of a staged iteration: (16 + 4 s)^2 records per array, rows padded to 8 mod 16 records (128 mod 256 bytes),
// which spreads the four rows a 16-lane read group touches over the 64 banks
__host__ __device__ inline int rt_denoise_lds_width(int step) { return RT_DENOISE_TILE + 4 * step; }
__host__ __device__ inline int rt_denoise_lds_stride(int step) { return ((rt_denoise_lds_width(step) + 7) & ~15) + 8; }
inline size_t rt_denoise_lds_bytes(int step, bool guide) {
    return (size_t)rt_denoise_lds_stride(step) * rt_denoise_lds_width(step) * sizeof(float4) * (guide ? 2 : 1);
}
hipError_t rt_launch_denoise_pack(const rt_denoise_params& dp, bool guide, hipStream_t st);
// staged: the tile and its 2 s halo through LDS (step <= RT_DENOISE_MAX_STAGED_STEP), else every tap through L1/L2
hipError_t rt_launch_denoise(bool normal_on, bool depth_on, bool color_on, bool staged, const rt_denoise_params& dp, hipStream_t st);

// rt_upscale (rt_kernel_upscale.hip): one launch, the pointers already checked on the host.  The denoiser's workgroup: 256
// threads on a 16x16 tile of the output, one output pixel per lane.
struct rt_upscale_params {
    const float* color_lo;    // ly * lx * 3
    const float* albedo_lo;   // null unless `demodulate`
    const float* normal_lo;   // null unless the normal factor is on
    const float* depth_lo;    // null unless the depth factor is on
    const float* albedo;      // ny * nx * 3, null unless `demodulate`
    const float* normal;      // ny * nx * 3, as normal_lo
    const float* depth;       // ny * nx, as depth_lo
    float* out;               // ny * nx * 3
    float* weight_out;        // ny * nx or null
    int32_t nx, ny;           // the output
    int32_t lx, ly;           // the coarse frame: nx / factor, ny / factor
    int32_t factor;
    int32_t tiles_x;          // 16x16-pixel workgroup tiles per row band of the output
    int32_t normal_sharpness; // m
    int32_t demodulate;
    float sigma_depth;
    float min_weight;
};
// The coarse records a tile's taps reach: columns x0 / f - 1 .. (x0 + 15) / f + 1, at most 16 / 2 + 3 = 11 (f >= 2), and as many
// rows.  The staged variant keeps them in static LDS, 11 x 11 records of 16 bytes in each of two arrays (3872 bytes).
#define RT_UPSCALE_WINDOW 11
// staged: the window through LDS, prepared once per workgroup; else every tap is read and prepared through L1/L2
hipError_t rt_launch_upscale(bool normal_on, bool depth_on, bool staged, const rt_upscale_params& up, hipStream_t st);

// rt_render_adaptive (rt_kernel_adaptive.hip): after each pass, one lane per pixel of that pass decides whether the pixel has
// converged at checkpoint n (include/rt_abi.h), writes the converged ones to fb / spp and appends the others -- wave-aggregated
// -- to list_out (local pixel ids, the main kernel's pixel list) and queue_out ((n << 32) | pixel, the tier kernel's tail queue).
enum { RT_ADAPTIVE_SNAPSHOT = 0,   // record h = the average at n for every pixel of the pass, decide nothing
       RT_ADAPTIVE_DECIDE = 1,     // the criterion at checkpoint n
       RT_ADAPTIVE_FINAL = 2 };    // n = max_spp: every pixel of the pass is written
#define RT_ADAPTIVE_THREADS 256
struct rt_adaptive_params {
    const rt_pixel_state* state;          // pixels parked at n samples
    float* half;                          // per pixel: the linear average at the previous checkpoint (3 floats)
    const uint32_t* list_in;              // the pass's pixels; null = local pixels [0, n_in)
    uint32_t n_in;
    uint32_t* list_out;                   // DECIDE: the next pass's pixels ...
    unsigned long long* queue_out;        // ... and the same as tail-queue entries
    uint32_t* count_out;                  // ... appended at this head
    float* fb;                            // compact local rows, nx * 3 floats each
    int32_t* spp;                         // final sample count per local pixel; null = not written
    int32_t n;                            // the checkpoint: samples in state
    int32_t mode;
    int32_t nx;
    float threshold, floor, gamma;
};
hipError_t rt_launch_adaptive(const rt_adaptive_params& p, hipStream_t st);

// rt_denoise_variance (rt_kernel_denoise.hip): the variance-guided mode of the filter.  The fourth float of the colour record
// carries the pixel's variance v_k instead of the colour sum (only the colour factor, which is off in this mode, reads that
// sum), so a tap still costs two 16-byte reads and the workspace is rt_denoise's.  Its kernels are entry points of rt_denoise's one
// iteration body; these arguments are a second block that only they take, so rt_denoise's own kernels reserve nothing for it.
struct rt_denoise_variance_params {
    const float* variance;    // pack: ny * nx, what rt_render_variance writes
    float* variance_out;      // last iteration: ny * nx, the filtered variance; null = not written
    float sigma_variance;
    float variance_floor;
};
hipError_t rt_launch_denoise_pack_variance(const rt_denoise_params& dp, const rt_denoise_variance_params& dv, bool guide, hipStream_t st);
hipError_t rt_launch_denoise_variance(bool normal_on, bool depth_on, bool staged, const rt_denoise_params& dp, const rt_denoise_variance_params& dv,
                                      hipStream_t st);

// rt_render_variance (rt_kernel_variance.hip): after pass b of B, one lane per local pixel reads the pixel's parked colour sum at
// c_b samples, forms the frame's float m_b as store_pixel does and updates the pixel's batch-means accumulators (include/rt_abi.h);
// the last pass also writes the frame and the variance.
#define RT_VARIANCE_THREADS 256
struct rt_variance_params {
    const rt_pixel_state* state;          // pixels parked at c samples
    double* acc;                          // per local pixel: T_{b-1}, A, Q
    float* fb;                            // last pass: compact local rows, nx * 3 floats each
    float* variance;                      // last pass: compact local rows of nx floats
    uint32_t n_pixels;
    int32_t c;                            // c_b: samples in state
    int32_t per;                          // n / B
    int32_t batches;                      // B
    int32_t first, last;                  // b == 1, b == B
    int32_t nx;
    float gamma;
};
hipError_t rt_launch_variance(const rt_variance_params& p, hipStream_t st);

// The finishing pass of rt_render and rt_render_window (rt_kernel_finish.hip): the main kernel and the tier kernel store each
// pixel's colour sum; this turns the frame's `floats` values into store_pixel's, in place: the scaling by 1 / ns, then gamma.
#define RT_FINISH_THREADS 256
hipError_t rt_launch_finish(float* fb, size_t floats, int32_t ns, float gamma, hipStream_t st);

// rt_render_aov_through (rt_kernel_aov_through.hip): the feature pass that follows the specular chain of every sample
// (include/rt_abi.h).  A second kernel argument beside rt_aov_params, which rt_kernel_aov.hip keeps as it is.
struct rt_aov_through_params {
    float* through;           // local_rows * nx; null = not written
    int32_t* bounces;         // local_rows * nx; null = not written
    int32_t max_bounces;
    float fuzz_limit;
};
// as rt_launch_aov / rt_aov_occupancy; grid = persistent workgroups of RT_AOV_THREADS
hipError_t rt_launch_aov_through(bool spheres_only, int tex_level, int lds_mode, const rt_scene_dev& sd, const rt_aov_params& ap,
                                 const rt_aov_through_params& tp, dim3 grid, size_t lds, hipStream_t st);
hipError_t rt_aov_through_occupancy(bool spheres_only, int tex_level, int lds_mode, size_t lds, int* blocks_per_cu);

// rt_reproject (rt_kernel_reproject.hip): the current frame blended into the reprojected history of the previous one
// (include/rt_abi.h), one lane per pixel, the pointers already checked on the host.  All buffers are planar, as the callers of
// rt_render_aov hold them.  history == null: the first frame (the four prev_* / history_len pointers are then not read).
#define RT_REPROJECT_THREADS 256
#define RT_REPROJECT_TILE 16
struct rt_reproject_params {
    const float* color;        // ny * nx * 3
    const float* depth;        // ny * nx
    const float* alpha;
    const float* normal;       // ny * nx * 3; read iff the normal test is on
    const int32_t* prim;       // read iff the id test is on
    const float* history;      // ny * nx * 3 or null
    const float* history_len;
    const float* prev_depth;
    const float* prev_alpha;
    const float* prev_normal;
    const int32_t* prev_prim;
    float* out;                // ny * nx * 3
    float* out_len;            // ny * nx
    float* motion;             // ny * nx * 2; written iff the motion output is on
    int32_t nx, ny, tiles_x, pad;
    float origin[3], lower_left[3], horizontal[3], vertical[3];   // of the current camera
    float prev_origin[3];
    float m[9];                // rt_reproject_matrix of the previous camera
    float alpha_min, depth_tol, normal_min, max_history;
};
// The follow step's tables, the kernel's optional second argument: each form's block extends the one before it, and the kernel of a
// form takes exactly its own block (rt_reproject's kernels take none).  A table is null exactly when its count is 0.
// Spheres (rt_reproject_moving): the sphere records of both frames and the media, whose boundaries say which sphere or instance a
// fog ball follows.
struct rt_reproject_follow_params {
    const rt_sphere* spheres;        // n_spheres records of the current frame
    const rt_sphere* prev_spheres;   // ... and of the previous frame, same order
    const rt_medium* media;          // n_media
    int32_t n_spheres, n_media;
    float time, prev_time;           // c = c0 + time * vel
};
// Instances (rt_reproject_instances): beside the sphere tables (n_spheres may be 0) the instance records of both frames and the two
// inst planes of rt_render_aov.  prev_inst is null exactly when rp.history is.
struct rt_reproject_follow_instance_params : rt_reproject_follow_params {
    const rt_instance* instances;        // n_instances records of the current frame
    const rt_instance* prev_instances;   // ... and of the previous frame, same order
    const int32_t* inst;                 // ny * nx, current
    const int32_t* prev_inst;            // ny * nx, previous
    int32_t n_instances, pad;
};
// Quads (rt_reproject_quads): beside the instance form (n_instances may be 0) the quad records of both frames.
struct rt_reproject_follow_quad_params : rt_reproject_follow_instance_params {
    const rt_quad* quads;        // n_quads records of the current frame
    const rt_quad* prev_quads;   // ... and of the previous frame, same order
    int32_t n_quads, pad_q;
};
// One launcher for the four entries.  `qp` is the full block, filled as far as `form` reaches.  ids_on is the static form's; the
// follow forms always test ids (their entries require prim and prev_prim).
enum rt_reproject_form { RT_REPROJECT_STATIC, RT_REPROJECT_SPHERES, RT_REPROJECT_INSTANCES, RT_REPROJECT_QUADS };
hipError_t rt_launch_reproject(rt_reproject_form form, bool normals_on, bool ids_on, bool motion_on, const rt_reproject_params& rp,
                               const rt_reproject_follow_quad_params& qp, hipStream_t st);

// rt_scene_update_spheres, _instances and _quads (rt_kernel_refit.hip; include/rt_abi.h): the replaced
// records, their leaves' boxes in every array that holds them, the per-64-leaf unions, the scene's coordinate bound and every
// interior box of both node arrays, as a few small launches on one stream.  The lookup tables are built by rt_abi.hip on a
// scene's first update.  One block serves the three kinds: `records`, `stamp` and `epoch` are those of the kind being updated
// (rt_refit::kind, rt_refit_host.h), everything else is the scene's.
#define RT_REFIT_THREADS 256
struct rt_refit_params {
    // the update: record k replaces record indices[k] of its kind (indices null: first + k); the indices were checked on the host
    const void* records;                  // rt_sphere, rt_instance or rt_quad: cast once, in the records kernel of the kind
    const int32_t* indices;
    int32_t count, first;
    int32_t n_materials;
    uint32_t epoch;                       // stamp[i] == epoch: record i was replaced by this update
    uint32_t* stamp;                      // per record of the kind; each kind has a stamp array and an epoch of its own
    // the scene's records (rt_scene_dev), writable: a records kernel stores into the array of its kind (a quad with pad0 = the
    // axis code), the marks kernel bit 30 of first_quad and nothing else; a leaf's box is computed from the records where they live
    rt_sphere* spheres;
    rt_instance* instances;
    rt_quad* quads;
    rt_box* boxes;
    int32_t n_boxes;
    // the leaves, by ordinal q (depth-first order, the same in both node arrays)
    int32_t n_leaves, n_slots;
    const int32_t* leaf_solid;            // the solid leaf q's box follows (its primitive or its medium's boundary), or -1
    const int32_t* leaf_node_ref;         // leaf q's index in nodes_ref ...
    const int32_t* leaf_node_walk;        // ... and in the walk array
    float4* box_lo;                       // canonical leaf boxes, padded to whole slots (padding: zeros, in no union)
    float4* box_hi;
    float4* tier_lo;                      // rt_scene_dev.leaf_lo / leaf_hi, or null: xyz follow, .w is not written
    float4* tier_hi;
    rt_node* nodes_ref;
    rt_node* nodes_walk;                  // null when the scene walks nodes_ref itself
    float* slot_box;                      // per slot 8 floats: lo, hi, 0, 0 (rt_scene_dev.slot_ranges when the scene has tier data)
    float* slot_abs;                      // per slot 4 floats: max(|lo|, |hi|) per axis over its leaves
    // one job per interior node of either array: (node index, first leaf, end leaf, 0 = nodes_ref / 1 = walk array)
    const int4* jobs;
    int32_t n_jobs;
    float* result;                        // [0..2] the scene's bound, [3] (as uint32) != 0: a record was refused on the device
};
// kind: rt_refit::kind.  Records, (quads: box marks,) leaves, slots, interior
hipError_t rt_launch_refit(const rt_refit_params& p, int kind, hipStream_t st);
