// rt_frame_plan.h -- what a render entry decides before its first enqueue (rt_abi.hip): the main kernel's launch
// shape, the tier kernel's room, the tier sizes and, for rt_render / rt_render_window, the whole frame's schedule as a value --
// its parts in order, what each is ranked on, which buffers it needs.  Host only and plain C++: no HIP call, no global, no scene;
// the functions read a plan_facts and an rt_options.  rt_abi.hip enqueues what a plan says; tests/frame_plan_check.cpp checks the
// rules here on a CPU.  The schedule is scheduling only -- every sample of every pixel is rendered once, in its stream order,
// whatever is decided here -- so the frames cannot show a wrong decision: that program and tools/launch_shapes.py do.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rt_device.h"
#include "rt_handoff_order.h"

// Tuning knobs (rt_set_option); rt_reset_options() restores exactly these defaults, which are what ships.
struct rt_options {
    int kernel = RT_KERNEL_STAGED;
    int lds_mode = -1;          // -1 = choose from the scene size
    int steps_per_trip = 12;
    int shade_threshold = 0;     // lanes with a finished walk that trigger stage C; 0 = 32, or 16 where the launch has less than 2.75 pixels per
                                 // resident lane (a share of a frame: waiting for a stage's quorum costs chain time there; 1/8: 50.0 -> 47.6 ms, 1/4: 62.1 -> 60.2)
    int wg_per_cu = 0;          // workgroups per CU of the staged kernel; 0 = per kernel family (2 x 512 lean, 3 x 256 otherwise)
    int threads = 0;            // workgroup size of the staged kernel; 0 = what the kernel family's register budget calls for
    int leaf_threshold = 8;     // lanes with an object test due that trigger the leaf pass (they keep walking meanwhile)
    int diel_threshold = 2;
    int box_threshold = 8;
    int medium_threshold = 16;
    int newpath_threshold = 0;   // lanes waiting for a new path before stage E runs; 0 = by kernel family: 24 spheres-only, 8 general (measured: Book-2 final 382 -> 364 ms with 8, Book-1 32.2 -> 35.1)
    int sparse_stride = 8;      // lanes per pixel in sparse waves (64 / live lanes); 0 disables sparse waves
    int split_samples = 16;      // samples per pixel rendered before pixels are ranked by measured cost (round 3: 16 and no presplit -- two parts; was 32 after a first look at 8)
    int tier_auto = 1;           // size the tiers from the share of the frame this call renders (effective_tier_sizes); 0 = the knobs as set
    int tier_kernel = 1;         // tier 1 of the list goes to the tier kernel (rt_kernel_tier.h) on a side stream; 0 = no tier 1
    int prior = 1;               // the first part of a split frame is already ranked: on the cost prior of the calibration frame
    int resplit_samples = 0;     // a second ranking: samples [split, resplit) run with tiers ranked on `split` samples, the rest ranked on `resplit` (0 = off)
    int presplit_samples = 0;    // a first, shorter look: samples [presplit, split) already run with tiers ranked on it (0 = off).  Off since the
                                 // cost prior ranks the first part: [0,16) + [16,ns) is as fast or faster than [0,8) + [8,32) + [32,ns) on every
                                 // BASELINE frame and 10 % faster at 100 spp (profiles/r03_two_parts.log)
    int tier1_factor_x10 = 45;   // tier 1 = heavy pixels costing >= this/10 x the mean
    int tier1_pixels = 1536;     // heavy pixels served one per wave at a time (tier 1)
    int cost_smooth_percent = 0;  // ranking: a pixel's cost estimate is at least this share of its dearest 4-neighbour's (0 = own cost only)
    int tier1_depth = 3;         // ... each wave taking about this many of them, one after the other
    int heavy_factor_x10 = 20;   // a pixel is listed ("heavy") when its cost so far is >= this/10 x the mean ...
    int sparse_factor_x10 = 40;  // ... and goes to a sparse wave (tier 2) from this/10 x the mean; below, ordinary lanes take it first (tier 3)
    int heavy_max_tiles = 0;     // 0 = as many as the sparse workgroups hold at once
    int semi_stride = -1;        // lanes per pixel in the workgroups serving tier 3 (0 = ordinary lanes take tier 3 first); -1 = by kernel family:
                                 // lean 1 -- whole waves of tier-3 pixels, which with semi_priority 1 measured 100.2 -> 94.3 ms on the headline
                                 // (profiles/r03_priorities_whole.log) --, the others 0 (Book-2 final 352 -> 388 ms with 1, profiles/r03_general_defaults.log)
    int sparse_priority = 3;
    int tier_priority = 1;       // s_setprio level of the tier kernel's waves (1 instead of 3: 80.6 -> 76.3 ms on a half, 70.2 -> 62.7 on a quarter of
                                 // the headline frame, nothing on the whole frame or an eighth: profiles/r03_share_sweep_pass2.log)
    int semi_priority = 1;       // s_setprio level of the semi workgroups' waves (tier 3 on workgroups of its own)
    int handoff = 1;             // tail hand-off (rt_device.h): the main kernel's last pixels are finished by a launch of the tier kernel after it
    int handoff_scan = 1;        // ... also in scenes scanned in lockstep (lds_mode 4), which have no tier 1
    int handoff_poll_us = 1000;  // ... looked for this often by each wave that has run out of queued work
    int handoff_pixels = -1;     // ... when at most this many are in flight and the tile queue is dry; -1 = auto (plan_frame)
    int handoff_order = 1;       // ... served most remaining work first: the queue is ordered on the device before the tail launch (rt_handoff_order.h); 0 = push order
    int sparse_eager = 0;
    int sparse_work_percent = 5;  // tiers 0-2 hold at most this share of the frame's work (rays so far); dearer-than-average pixels beyond it go to tier 3
    int sparse_wg_percent = 35;   // at most this share of the workgroups starts in sparse mode
    int bvh_collapse = 3;        // walk array (rt_scene_create): 0 = the reference's tree as is, 1 = interior nodes that do not pay
                                 // removed, decided from box surface areas, 2 = decided from pass counts measured on a small frame,
                                 // 3 = as 2, and the leaves regrouped by surface-area cost if that predicts fewer box tests
    int scan_nodes = 24;         // scenes whose walk array has at most this many nodes are scanned in lockstep (lds_mode 4); 0 = never
    int multi_force_rccl = 0;    // rt_multi_render: go through the RCCL gather even with one device (tests the path on a one-GPU box)
    int lpt = 1;                 // cost prepass + longest-first tile order (staged kernel, ns >= 2 * split_samples)
    int cost_map = 1;            // ranked frames leave and use the scene's cost map (struct rt_scene); 0 = neither
    int trace_lds = -1;          // rt_trace_rays: -1 = auto, 0 = scene through L1/L2, 1 = nodes in LDS, 2 = nodes and spheres in LDS
    int trace_tree = 1;          // rt_trace_rays: 1 = the walk array, 0 = the reference's full tree
    int radiance_lds = -1;       // rt_radiance_rays: as trace_lds
    int aov_lds = -1;            // rt_render_aov: as trace_lds
    int aov_through_lds = -1;    // rt_render_aov_through: as trace_lds
    int denoise_lds = -1;        // rt_denoise: -1 = iterations with taps up to 4 pixels apart stage tile + halo in LDS, 0 = never,
                                 // 1 = wherever the tile fits (taps up to 8 apart)
    int upscale_lds = -1;        // rt_upscale: -1 (auto) and 1 = the coarse pixels a tile reaches are prepared once in LDS, 0 = every
                                 // tap is read through L1/L2
    int adaptive_tier = -1;      // rt_render_adaptive: -1 = a pass goes to the tier kernel when its active pixels fit the tier waves at once
                                 // (DESIGN.md 4.8), 0 = always the main kernel, 1 = the tier kernel wherever the scene's tier data fit
};

// The facts a plan reads about the device and the scene (rt_host.h fills them in one place, plan_facts_of).
struct plan_facts {
    int num_cu;
    size_t lds_per_cu;
    bool spheres_only;
    int tex_level;
    size_t node_bytes, sphere_bytes, shade_bytes;   // node_bytes: the walk array; shade_bytes: materials + textures
    int n_nodes;                                    // of the walk array
    bool tier_data;                                 // the scene has the tier kernel's leaf arrays
    int n_slots, n_spheres, n_materials, n_textures;
    bool calibrated;                                // a calibration prior exists
    size_t handoff_capacity;                        // entries the scene's hand-off queue holds already (buffers only grow)
    // the lean spheres-only kernels (2 x 512 threads per CU) as against the others (3 x 256)
    bool lean_family() const { return spheres_only && tex_level < 2; }
};

// What a call renders of the frame `f` describes: its rows of the partition, its grid of 8x8 tiles, and the pixels and work items
// (64 per tile) in them.
struct frame_geometry {
    int local_rows, tiles_x, tiles_y;
    size_t n_pixels;
    uint32_t work_items;
};

// What a cost map was measured for (struct rt_scene): the frame geometry, the row partition and the kernel.
struct cost_map_key {
    int32_t nx = 0, ny = 0, tile_rows = 0, tile_first = 0, tile_stride = 0, local_rows = 0, kernel_variant = 0;
    bool operator==(const cost_map_key& o) const {
        return nx == o.nx && ny == o.ny && tile_rows == o.tile_rows && tile_first == o.tile_first && tile_stride == o.tile_stride &&
               local_rows == o.local_rows && kernel_variant == o.kernel_variant;
    }
};
// ... and what a plan reads of the scene's map: whether it holds a closed frame's costs, of which view, and the scene's and the
// options' epochs then and now
struct cost_map_view {
    bool valid, has_total;
    cost_map_key key;
    unsigned long long scene_epoch, opt_epoch, scene_epoch_now, opt_epoch_now;
};

// The main kernel's launch shape for a launch over `n_pixels` pixels (`work_items` work items): LDS residency mode, workgroup
// shape, grid and stage quorums.  Shared by rt_render / rt_render_window and rt_render_adaptive's passes.
struct main_launch {
    int kernel, lds_mode;
    size_t lds_bytes;
    dim3 grid, block;
    int per_cu_resident;   // workgroups of this launch that can be resident on one CU (persistent kernels)
    int shade_threshold, newpath_threshold;   // the stage quorums (rt_frame_params)
};
// `why`: the text of the one refusal (status RT_ERR_INVALID)
inline rt_status plan_main_launch(const plan_facts& c, const rt_options& o, int kernel, size_t n_pixels, uint32_t work_items, main_launch& ml, const char*& why) {
    // LDS residency: nodes + spheres in every workgroup of a CU if they fit that many times (2 workgroups for the lean
    // spheres-only kernels, 3 otherwise: see the workgroup shapes below), else once (one big workgroup per CU), else nodes only
    int lds_mode = o.lds_mode;
    const bool lean_family = c.lean_family();
    const size_t budget1 = c.lds_per_cu - 2048;   // one workgroup per CU
    // the staged kernel's image of the nodes carries a word per record behind them (the leaves' object references: rt_device.h)
    const size_t image_bytes = c.node_bytes + (kernel == RT_KERNEL_STAGED ? (size_t)RT_WALK_PRIM_TABLE_BYTES(c.n_nodes) : 0);
    if (lds_mode < 0) {
        // nodes + spheres where they fit a CU at all (several workgroups each with its own image, or one big workgroup
        // sharing one: see the workgroup shapes below), else nodes only, else everything through L1 / L2
        // (lds_mode 3 -- materials and textures in LDS too -- is selectable but measured no faster: profiles/r01_sweep34)
        if (image_bytes + c.sphere_bytes <= budget1) lds_mode = 2;
        else if (image_bytes <= budget1) lds_mode = 1;
        else lds_mode = 0;
    }
    if (o.lds_mode < 0 && kernel == RT_KERNEL_STAGED && o.scan_nodes > 0 && c.n_nodes <= o.scan_nodes) lds_mode = 4;   // lockstep scan of a tiny scene
    if (lds_mode >= 3 && kernel != RT_KERNEL_STAGED) lds_mode = 2;
    if (kernel == RT_KERNEL_PIXEL) lds_mode = 0;   // the cross-check kernel reads the scene through L1/L2
    size_t lds_bytes = 0;
    if (lds_mode >= 1 && lds_mode <= 3) lds_bytes += image_bytes;
    if (lds_mode >= 2 && lds_mode <= 3) lds_bytes += c.sphere_bytes;
    if (lds_mode == 3) lds_bytes += c.shade_bytes;
    if (lds_bytes > budget1) { why = "requested lds_mode does not fit the CU's LDS"; return RT_ERR_INVALID; }
    dim3 grid, block;
    int per_cu_resident = 1;   // workgroups of this launch that can be resident on one CU (persistent kernels)
    if (kernel == RT_KERNEL_PIXEL) {
        block = dim3(256);
        grid = dim3((work_items + 255u) / 256u);
    } else {
        // workgroup shape per kernel family (register budgets: launch bounds, rt_device.h): the lean spheres-only
        // kernels 2 x 512 threads per CU (4 waves per SIMD), the others 3 x 256 (3 waves per SIMD; workgroups of four
        // waves, one per SIMD -- 2 x 384 threads is the same occupancy and measured 1.4x slower on the Cornell box)
        const bool lean = lean_family;
        const int fam_max_threads = lean ? RT_LEAN_MAX_THREADS : RT_HEAVY_MAX_THREADS;
        const int lds_fit = lds_bytes ? (int)(c.lds_per_cu / (lds_bytes + 512)) : 8;
        int per_cu = o.wg_per_cu > 0 ? o.wg_per_cu : (lean ? 2 : 3);
        int threads = o.threads > 0 ? o.threads : (lean ? 512 : 256);
        if (o.wg_per_cu <= 0 && o.threads <= 0 && lds_fit < per_cu) {
            // the scene's LDS image does not fit that many times: one workgroup with all the CU's waves shares one image
            per_cu = 1; threads = fam_max_threads;
        }
        if (lds_fit < per_cu) per_cu = lds_fit < 1 ? 1 : lds_fit;
        if (threads > fam_max_threads) threads = fam_max_threads;
        if (threads < 64) threads = 64;
        block = dim3((unsigned)threads);
        unsigned want = (unsigned)(c.num_cu * per_cu);
        const unsigned need = (work_items + (unsigned)threads - 1) / (unsigned)threads;
        grid = dim3(want < need ? want : need);
        per_cu_resident = per_cu;
    }
    {   // stage quorums.  In a launch that leaves the machine mostly empty (a small share of a frame) a lane waiting for 32 others
        // to finish their walks is waiting on the frame's critical path: the quorums are halved there.
        const double pixels_per_lane = (double)n_pixels / ((double)c.num_cu * (double)per_cu_resident * (double)block.x);
        // (lean family: every share of the BASELINE frames -- a whole frame is 3.3 - 3.7; the Cornell box's 1/8 share is slower with them: 172 -> 179 ms)
        const bool latency_regime = kernel == RT_KERNEL_STAGED && lean_family && pixels_per_lane < 2.75;
        ml.shade_threshold = o.shade_threshold > 0 ? o.shade_threshold : (latency_regime ? 16 : 32);
        ml.newpath_threshold = o.newpath_threshold > 0 ? o.newpath_threshold : (c.spheres_only ? (latency_regime ? 12 : 24) : 8);
    }
    ml.kernel = kernel; ml.lds_mode = lds_mode; ml.lds_bytes = lds_bytes; ml.grid = grid; ml.block = block; ml.per_cu_resident = per_cu_resident;
    return RT_OK;
}
// the kernel and its instantiation as rt_stats reports them and the cost map is keyed on them
inline int kernel_variant_of(const plan_facts& c, const main_launch& ml) {
    return ml.kernel * 1000 + ml.lds_mode * 100 + c.tex_level * 10 + (c.spheres_only ? 1 : 0);
}

// Room for the tier kernel (rt_kernel_tier.h) in `budget` bytes of LDS per workgroup: whether its image fits -- the scene has
// tier data, and the leaf arrays, which the image always holds, fit --, whether spheres, materials and textures fit too
// (rt_frame_params::tier_lds_scene), the image's size, and the grid of a tail launch.
// The tail launch has the machine to itself: as many tier workgroups per CU as registers (launch bounds: 4 resp. 3 waves per SIMD,
// a workgroup is one wave per SIMD) and LDS hold
struct tier_room {
    bool fits;
    int lds_scene;
    size_t lds;
    unsigned tail_grid;
};
inline tier_room plan_tier_room(const plan_facts& c, size_t budget) {
    tier_room r = {false, 0, 0, 0};
    const int ns_ = c.n_slots, nsph = c.n_spheres, nm = c.n_materials, nt = c.n_textures;
    if (!c.tier_data || rt_tier_lds_bytes(ns_, nsph, nm, nt, false) > budget) return r;
    r.fits = true;
    r.lds_scene = rt_tier_lds_bytes(ns_, nsph, nm, nt, true) <= budget ? 1 : 0;
    r.lds = rt_tier_lds_bytes(ns_, nsph, nm, nt, r.lds_scene != 0);
    const unsigned by_lds = (unsigned)(c.lds_per_cu / (r.lds + 512));
    const unsigned by_regs = c.lean_family() ? 4u : 3u;
    r.tail_grid = (unsigned)c.num_cu * (by_lds < by_regs ? by_lds : by_regs);
    if (r.tail_grid < 1u) r.tail_grid = 1u;
    return r;
}

struct tier_sizes { int tier1_pixels, tier1_factor, tier1_depth, heavy_factor, sparse_factor, sparse_percent, work_percent; };
inline tier_sizes effective_tier_sizes(double per_lane, bool lean_family, const rt_options& o) {
    // Effective tier sizes by the share of the frame this call renders (1/N in an N-GPU run): the fewer pixels a
    // rank has per lane, the more of them can afford a wave of their own.  Measured on rank-local renders of the
    // headline frame (tools/partition_time.py).
    int e_tier1_pixels = o.tier1_pixels, e_tier1_factor = o.tier1_factor_x10, e_tier1_depth = o.tier1_depth,
        e_heavy_factor = o.heavy_factor_x10, e_sparse_factor = o.sparse_factor_x10, e_sparse_percent = o.sparse_wg_percent,
        e_work_percent = o.sparse_work_percent;
    if (o.tier_auto) {
        // keyed by pixels per resident lane (the 1200x800 frame: 3.7 whole, 1.8 / 0.9 / 0.5 for a half, a quarter,
        // an eighth; a quarter of 1920x1080 is 2.0): what matters is how empty the machine is, not the fraction
        if (per_lane > 2.75) {
            // whole frames.  Lean family: the defaults.  The others: a tier wave is a main workgroup's slot taken away and
            // their dear pixels are many and alike (Book-2 final: the fog ball), so only the very dearest get one
            // (Book-2 final 800x800 @ 200: 352 ms with the lean sizes, 342 ms with these, profiles/r03_general_defaults.log)
            if (!lean_family) { e_tier1_factor = 70; e_tier1_pixels = 256; e_tier1_depth = 1; }
        }
        // shares, lean family: re-fitted in round 3 with the tier kernel beside the main kernel (tools/share_sweep.py on rank 0
        // of the 1200x800 and 1920x1080 frames, profiles/r03_share_sweep_pass*.log; slowest-rank tables in DESIGN.md section 6)
        // -- and again with the tail hand-off, which takes over what the largest tiers were there for (rank 0 of 8: 48.1 ms with
        // round 3's first fit 16384 / 1.5x, 40.6 ms with the quarter's sizes; rank 0 of 2: 66.2 -> 62.6 ms, profiles/r03_handoff_shares.log)
        else if (lean_family) {
            if (per_lane > 1.375) { e_tier1_pixels = 1536; e_tier1_factor = 40; e_tier1_depth = 3; e_heavy_factor = 20; e_sparse_factor = 40; e_sparse_percent = 80; e_work_percent = 5; }
            else { e_tier1_pixels = 8192; e_tier1_factor = 20; e_tier1_depth = 4; e_heavy_factor = 15; e_sparse_factor = 20; e_sparse_percent = 80; e_work_percent = 40; }
        }
        // shares, other families: round 2's sizes (Book-2 final's 1/8 share: 216 ms with these, 236 with the lean family's,
        // 252 without a tier kernel, profiles/r03_share_sweep_final_eighth.log)
        else if (per_lane > 1.375) { e_tier1_pixels = 4096; e_tier1_factor = 30; e_tier1_depth = 4; e_heavy_factor = 20; e_sparse_factor = 30; e_sparse_percent = 80; }
        else if (per_lane > 0.6875) { e_tier1_pixels = 4096; e_tier1_factor = 30; e_tier1_depth = 4; e_heavy_factor = 20; e_sparse_factor = 30; e_sparse_percent = 80; e_work_percent = 20; }
        else { e_tier1_pixels = 8192; e_tier1_factor = 20; e_tier1_depth = 4; e_heavy_factor = 15; e_sparse_factor = 15; e_sparse_percent = 80; e_work_percent = 40; }
    }
    if (e_sparse_factor < e_heavy_factor) e_sparse_factor = e_heavy_factor;
    return {e_tier1_pixels, e_tier1_factor, e_tier1_depth, e_heavy_factor, e_sparse_factor, e_sparse_percent, e_work_percent};
}

// rt_render_adaptive's tier route: whether a pass over `active` pixels goes to the tier kernel's tail mode, given its room
// (plan_tier_room in lds_per_cu - 2048 bytes).
// auto crossover: a pass goes to the tier kernel when it has at most this many active pixels per resident tier wave.  Measured
// on row shares with every pixel active (tools/adaptive_sweep.py --config crossover, profiles/adaptive_mi355x.jsonl, DESIGN.md
// 4.8): the Cornell box's routes tie at 22 800 pixels (7.4 per wave of 3 072); on the headline scene the tier route is 1.6x
// faster at 60 000 pixels and still 10 % faster at 107 500 (26 per wave of 4 096), and 1.5x slower at 240 000
inline bool adaptive_use_tier(const plan_facts& c, const tier_room& room, const rt_options& o, uint32_t active) {
    if (!room.fits || o.adaptive_tier == 0) return false;
    if (o.adaptive_tier == 1) return true;
    const size_t tier_waves = (size_t)room.tail_grid * (RT_TIER_THREADS / 64);
    const size_t tier_per_wave = c.lean_family() ? 32 : 6;
    return (size_t)active <= tier_per_wave * tier_waves;
}

// ---- the frame's schedule (rt_render, rt_render_window)
// what a part's tiles and tiers are ranked on: nothing (the plain grid), a prior written into d_state and d_tile_cost -- the
// calibration frame's, or the cost map's, their sum in d_ray_counter[3] --, or the rays measured so far (d_ray_counter[0])
enum part_rank { RANK_NONE, RANK_CALIBRATION, RANK_MAP, RANK_MEASURED };
// One part of a frame: samples [sample_begin, sample_end) of every local pixel.  `state` below is the scene's d_state, or in a
// progressive window the caller's.
struct frame_part {
    int32_t sample_begin, sample_end;
    part_rank ranked_on;
    bool fresh;              // its pixels start afresh although state_in is set (it holds the prior's costs only)
    bool reads_state;        // state_in: pixels are resumed from the state (or, fresh, ranked on the costs there)
    bool parks_state;        // state_out: pixels are parked at sample_end
    bool writes_tile_cost;   // adds its rays to d_tile_cost
    bool clear_before;       // d_tile_cost is cleared first (before the prior, if there is one) ...
    bool clear_after;        // ... and again behind the ranking: from there on it holds measured rays
    unsigned grid;           // of the main kernel
    bool tiers;              // tier 1 runs beside it: the tier kernel on its own stream
    bool tail;               // it hands its last pixels off through d_state and a tail launch follows it
    int32_t cost_begin;      // first sample the parked costs cover (the ordering launch: rt_handoff_order.h)
};
enum { RT_MAX_FRAME_PARTS = 4 };   // parts 1, 1b, 1c and the last
struct sample_window { bool on; int32_t begin, end; };   // rt_render_window's [begin, end); off: the whole frame
// Everything render_impl decides before its first enqueue.
struct frame_plan {
    int kernel = 0;
    main_launch ml = {};
    int kernel_variant = 0;
    // the tier kernel beside ranked parts (tier 1), and behind every part of a ranked frame (tail launches)
    bool tier_possible = false;
    unsigned tier_grid = 0;
    int tier_waves_per_main_wg = 0;
    tier_room room = {false, 0, 0, 0};   // fits: enough for the tail launches (tail hand-off) even where tier 1 is not used
    unsigned tail_grid = 0;
    bool ranked = false;                 // the cost-aware schedule
    // the hand-off (ranked frames with a tail grid; handoff_capacity 0: none)
    size_t handoff_capacity = 0;         // entries the queue must hold
    int32_t handoff_pixels = 0, handoff_poll_ticks = 0;
    bool tail_ordered = false;
    uint32_t order_min = 0, order_max = 0;
    // the rankings (rt_rank_params)
    unsigned max_grid = 0, normal_need = 0;
    tier_sizes sizes = {};
    int sparse_stride = 0, semi_stride = 0, smooth_percent = 0;
    // the cost map
    cost_map_key key;                    // of this frame (ranked frames)
    bool map_usable = false, map_exact = false;
    bool cost_out = false;               // the last part's launches write the next map
    // element counts of the scene's buffers this frame needs (0: not needed)
    size_t ranked_tiles = 0, ranked_pixels = 0, cost_map_pixels = 0, handoff_ordered_capacity = 0, handoff_scratch_words = 0;
    int n_parts = 0;
    frame_part parts[RT_MAX_FRAME_PARTS] = {};
    int ranked_parts = 0;                // parts of the last RANKED frame (render_impl carries it over an unranked one)
};

inline frame_part& add_part(frame_plan& p, int32_t begin, int32_t end) {
    frame_part& part = p.parts[p.n_parts++];
    part = frame_part();
    part.sample_begin = begin; part.sample_end = end;
    part.ranked_on = RANK_NONE;
    return part;
}
// a ranked part between two others: samples [begin, end) of every pixel, resumed from and parked into d_state, with
// tiers ranked on the rays measured so far
inline void add_middle_part(frame_plan& p, int32_t begin, int32_t end) {
    frame_part& part = add_part(p, begin, end);
    part.ranked_on = RANK_MEASURED;
    part.reads_state = part.parks_state = part.writes_tile_cost = true;
}

inline rt_status plan_frame(const plan_facts& c, const rt_options& o, const rt_frame_desc& f, const frame_geometry& g, const sample_window& win,
                            const cost_map_view& cm, frame_plan& p, const char*& why) {
    p = frame_plan();
    const int32_t frame_ns = win.on ? win.end : f.ns;
    p.kernel = win.on ? RT_KERNEL_STAGED : o.kernel;   // (kernel 0 renders whole pixels only)
    const rt_status st = plan_main_launch(c, o, p.kernel, g.n_pixels, g.work_items, p.ml, why);
    if (st != RT_OK) return st;
    const main_launch& ml = p.ml;
    p.kernel_variant = kernel_variant_of(c, ml);
    const bool lean_family = c.lean_family();
    const int per_cu_resident = ml.per_cu_resident;

    // ---- tier room.  The tier kernel of ranked launches (rt_kernel_tier.h): its LDS image and where its workgroups find room.
    // Lean family: the main kernel's 4 x 104 registers per SIMD leave 96 free, so ONE tier workgroup (four waves, one per
    // SIMD, 76 VGPRs) is resident on a CU beside a full main grid if the LDS left over holds its image.  Other families:
    // no register room beside a full main grid; the ranking makes main workgroups leave (main_skip_wgs) and a tier workgroup
    // has what one of them had.  The image always holds the leaf arrays; spheres, materials and textures too where all of them fit.
    if (p.kernel == RT_KERNEL_STAGED && (o.tier_kernel || o.handoff) && c.tier_data) {
        size_t budget;
        if (lean_family) {
            const size_t used = (size_t)per_cu_resident * (ml.lds_bytes + 512);
            budget = c.lds_per_cu > used + 1024 ? c.lds_per_cu - used - 1024 : 0;
        } else {
            // the slot of one main workgroup, shared by the tier workgroups it holds: as many as it has groups of four waves
            const unsigned tier_wgs_per_slot = ml.block.x / RT_TIER_THREADS > 0 ? ml.block.x / RT_TIER_THREADS : 1u;
            budget = (c.lds_per_cu / (size_t)per_cu_resident - 1024) / tier_wgs_per_slot;
            p.tier_waves_per_main_wg = (int)(tier_wgs_per_slot * (RT_TIER_THREADS / 64));
        }
        p.room = plan_tier_room(c, budget);
        if (p.room.fits) {
            // (not for scenes scanned in lockstep, lds_mode 4: a handful of leaves, every pixel about as dear as the next -- the Cornell
            // box's 1/8 share measured 182 ms without it and 199 ms with it, profiles/r03_general_defaults.log)
            p.tier_possible = o.tier_kernel && ml.lds_mode != 4 && o.tier1_pixels > 0;
            // the tier kernel's grid is fixed before the ranking has sized the tier: what can be resident beside the main
            // grid (one workgroup per CU) and as much again queued behind it; workgroups beyond the tier's size leave at once
            p.tier_grid = lean_family ? (unsigned)(2 * c.num_cu) : (unsigned)(c.num_cu * per_cu_resident) * (unsigned)(p.tier_waves_per_main_wg / (RT_TIER_THREADS / 64)) / 2u;
            if (p.tier_grid < 1u) p.tier_grid = 1u;
        }
    }
    p.tail_grid = p.room.fits && o.handoff && (ml.lds_mode != 4 || o.handoff_scan) ? p.room.tail_grid : 0u;

    const size_t n_tiles = (size_t)g.tiles_x * (size_t)g.tiles_y;
    const size_t n_pixels = g.n_pixels;
    if (win.on) {
        // a progressive window: one launch, every pixel resumed from (first window: started in) and parked into the caller's state,
        // and written to fb as the average so far
        frame_part& part = add_part(p, win.begin, win.end);
        part.reads_state = win.begin > 0; part.parks_state = true;
    } else if (o.lpt && p.kernel == RT_KERNEL_STAGED && f.ns >= 2 * o.split_samples && n_tiles >= 64 && n_pixels < (1ull << 31)) {
        p.ranked = true;
        p.ranked_tiles = n_tiles; p.ranked_pixels = n_pixels;
        // ---- the scene's cost map (struct rt_scene): exact -- this very view was rendered last, under these options --, stale, or of no use
        cost_map_key& key = p.key;
        key.nx = f.nx; key.ny = f.ny; key.tile_rows = f.tile_rows; key.tile_first = f.tile_first; key.tile_stride = f.tile_stride;
        key.local_rows = g.local_rows; key.kernel_variant = p.kernel_variant;
        if (o.cost_map) p.cost_map_pixels = n_pixels;   // (a map that has to grow for this frame was of another view: key)
        // The map is read by the lean family and by scenes without tier 1 (scanned in lockstep, or no tier data).  Where tier workgroups
        // take main workgroups' slots (the other families with tier 1) it is written and not read: Book-2 final 800x800 @ 200 measured
        // 246-249 ms in two parts and 251-262 ms in one (profiles/cost_map_mi355x.jsonl): its tier-1 chain
        // bounds the frame either way.
        const bool map_read = lean_family || !p.tier_possible;
        p.map_usable = o.cost_map && o.prior && map_read && cm.valid && cm.has_total && cm.key == key;
        p.map_exact = p.map_usable && cm.scene_epoch == cm.scene_epoch_now && cm.opt_epoch == cm.opt_epoch_now;
        p.cost_out = o.cost_map != 0;   // the last part's launches leave the next map; it counts from rt_frame_finish on
        if (p.tail_grid > 0) {
            // tail hand-off (rt_device.h): a lane hands off at most one pixel per launch, so the queue holds one entry per resident lane
            const size_t need = (size_t)c.num_cu * (size_t)per_cu_resident * (size_t)ml.block.x;
            p.handoff_capacity = c.handoff_capacity > need ? c.handoff_capacity : need;
            p.handoff_poll_ticks = o.handoff_poll_us * 100;
            // auto: six pixels per wave of the tail launch (the headline frame: 18432 of 960000; 8192 .. 32768 measure the same,
            // profiles/r03_handoff.log), and never more than 1/8 of the pixels (small frames and shares: the Cornell box's
            // 1/8 share, 45000 pixels, 178 ms without, 163 ms at 4096 - 8192, 180 ms at 16384).
            // Twelve per wave in the lean family when the tail is served most remaining work first (handoff_order): the tail ends with
            // its longest chain, not with its queue, so a larger hand-off moves that chain to a tier wave earlier -- headline 67.3 ms at
            // 6 in push order, 66.4 at 6 ordered, 65.0 - 65.1 at 10 - 12 ordered, 65.3 at 14, 66.1 at 16, and 67.7 at 12 in push order.
            // The other families stay at 6: their tier waves spill and gain less on a main lane (Cornell smoke 46.6 ms at 6, 48.2 at
            // 12; Cornell and Book-2 final measure the same at both; profiles/tail_order_mi355x.jsonl).
            const size_t tail_waves = (size_t)p.tail_grid * (RT_TIER_THREADS / 64);
            const size_t cap_px = n_pixels / 8;
            const size_t per_wave = (o.handoff_order && lean_family) ? 12 : 6;
            p.handoff_pixels = o.handoff_pixels >= 0 ? o.handoff_pixels : (int32_t)(per_wave * tail_waves < cap_px ? per_wave * tail_waves : cap_px);
            if (o.handoff_order) {
                // ordered between two and 32 entries per tail wave, copied through outside (rt_handoff_order.h)
                const size_t most = (size_t)RT_HANDOFF_ORDER_MAX_PER_WAVE * tail_waves;
                p.order_min = (uint32_t)(RT_HANDOFF_ORDER_MIN_PER_WAVE * tail_waves);
                p.order_max = (uint32_t)(most < p.handoff_capacity ? most : p.handoff_capacity);
                p.handoff_ordered_capacity = p.handoff_capacity;
                p.handoff_scratch_words = rt_handoff_order_scratch_words(p.order_max);
                p.tail_ordered = true;
            }
        }
        // ---- the rankings.  The grids are fixed here, before the tier sizes are known: the workgroups the ordinary queue needs plus
        // the most the sparse tier may take; a workgroup that finds both its queues empty leaves at once.
        p.max_grid = (unsigned)(c.num_cu * per_cu_resident);
        p.sizes = effective_tier_sizes((double)n_pixels / ((double)p.max_grid * (double)ml.block.x), lean_family, o);
        p.normal_need = (uint32_t)((g.work_items + ml.block.x - 1) / ml.block.x);
        p.sparse_stride = (o.sparse_stride > 0 && ml.block.x >= 64) ? o.sparse_stride : 0;
        p.semi_stride = o.semi_stride >= 0 ? o.semi_stride : (lean_family ? 1 : 0);
        p.smooth_percent = o.cost_smooth_percent;
        if (p.map_exact) {
            // ---- one part: the map holds what every pixel of this view cost over a whole frame, measured -- better than any first look of
            // this frame could -- so samples [0, ns) run as a single fresh part ranked on it: no parking, no second ranking, one tail
            frame_part& part = add_part(p, 0, frame_ns);
            part.ranked_on = RANK_MAP;
            part.clear_before = part.reads_state = part.fresh = true;
        } else {
            // ---- part 1: samples [0, S_a); S_a = presplit_samples, or S0.  Nothing has been measured yet; with the cost prior
            // (rt_prior_kernel: the calibration frame's rays per pixel, scaled to this frame) the part is ranked all the same,
            // so that the dearest chains start on tier waves at sample 0 instead of running at an ordinary lane's pace.
            const int first_end = (o.presplit_samples > 0 && o.presplit_samples < o.split_samples) ? o.presplit_samples : o.split_samples;
            frame_part& p1 = add_part(p, 0, first_end);
            p1.clear_before = p1.parks_state = p1.writes_tile_cost = true;
            // A stale map (the camera or a sphere has moved since, or an option was set) is still the better prior: measured, at this
            // frame's own resolution.
            if (p.map_usable || (o.prior && c.calibrated)) {
                p1.ranked_on = p.map_usable ? RANK_MAP : RANK_CALIBRATION;
                p1.reads_state = p1.fresh = true;
                p1.clear_after = true;   // from here on: measured rays
            }
            // ---- part 1b: samples [S_a, S0), with tiers ranked on the first S_a samples.
            if (first_end < o.split_samples) add_middle_part(p, first_end, o.split_samples);
            // ---- part 1c (optional): samples [S0, S1), ranked on the first S0 samples; the last part is then ranked again on
            // S1 samples.  A pixel's cost over 32 samples is a noisy estimate of its cost over 500 (paths through glass are
            // heavy-tailed): pixels that look cheap and are not start late and end the frame (tools/diag_wave_ends.py).
            int last_begin = o.split_samples;
            if (o.resplit_samples > o.split_samples && f.ns >= 2 * o.resplit_samples) {
                add_middle_part(p, o.split_samples, o.resplit_samples);
                last_begin = o.resplit_samples;
            }
            // ---- last part: samples [S1 or S0, ns), ranked on everything rendered so far
            frame_part& last = add_part(p, last_begin, frame_ns);
            last.ranked_on = RANK_MEASURED;
            last.reads_state = true;
        }
        p.ranked_parts = p.n_parts;
    } else {
        add_part(p, 0, frame_ns);
    }
    // a ranked part's grid: what the ordinary queue needs plus the most the sparse tier may take
    unsigned ranked_grid = p.normal_need + (p.sparse_stride > 0 ? p.max_grid * (unsigned)p.sizes.sparse_percent / 100u : 0u);
    if (p.tier_waves_per_main_wg > 0 && p.tier_possible) ranked_grid = p.max_grid;      // (workgroups that make room for the tier kernel are part of the grid)
    if (ranked_grid > p.max_grid) ranked_grid = p.max_grid;
    if (ranked_grid < 1u) ranked_grid = 1u;
    for (int k = 0; k < p.n_parts; ++k) {
        frame_part& part = p.parts[k];
        const bool is_ranked = part.ranked_on != RANK_NONE;
        part.grid = is_ranked ? ranked_grid : ml.grid.x;
        part.tiers = is_ranked && p.tier_possible;
        part.tail = p.handoff_capacity > 0;
        // The parked costs count from sample 0 except in a part that starts its pixels afresh.
        part.cost_begin = (part.reads_state && !part.fresh) ? 0 : part.sample_begin;
    }
    return RT_OK;
}
