// The frame plan (csrc/rt_frame_plan.h) on its own: what rt_render and its siblings decide before they enqueue anything, rule by
// rule.  Every expected value below is written out by hand from the rule the comment names; none is computed by the code under
// test.  tests/test_frame_plan_host.py builds this with -fsanitize=address,undefined and runs it; no HIP call, no device.
//
// The facts are synthetic: 256 CUs with 160 KiB (163 840 bytes) of LDS each, so `budget1` = 163 840 - 2 048 = 161 792, and a
// walk array of 100 nodes in 3 200 bytes, whose staged image carries a 400-byte prim table: 3 600 bytes.
#include <cstdio>
#include <cstring>

#include "rt_frame_plan.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static_assert(sizeof(rt_texture) == 64, "the lds_scene boundary below counts one 64-byte texture");
static_assert(RT_KERNEL_STAGED == 3 && RT_KERNEL_PIXEL == 0, "kernel_variant below");

// a scene of the lean family (spheres only, no noise or image texture) or of the others; `sphere_bytes` sets the LDS image's size:
// lds_bytes = 3 600 + sphere_bytes in lds_mode 2.  25 slots: a tier image of 25 * 2 080 = 52 000 bytes.
static plan_facts scene(bool lean, size_t sphere_bytes = 16000) {
    plan_facts c;
    std::memset(&c, 0, sizeof(c));
    c.num_cu = 256; c.lds_per_cu = 160 * 1024;
    c.spheres_only = lean; c.tex_level = 0;
    c.node_bytes = 3200; c.n_nodes = 100; c.sphere_bytes = sphere_bytes; c.shade_bytes = 1000;
    c.tier_data = true; c.n_slots = 25;
    c.calibrated = true;
    return c;
}
// the geometry of `rows` local rows of an nx-wide frame (what check_frame in rt_host.h computes)
static frame_geometry geometry(int nx, int rows) {
    frame_geometry g;
    g.local_rows = rows; g.tiles_x = (nx + 7) / 8; g.tiles_y = (rows + 7) / 8;
    g.n_pixels = (size_t)rows * nx; g.work_items = (uint32_t)(g.tiles_x * g.tiles_y * 64);
    return g;
}
static rt_frame_desc frame(int nx, int ny, int ns) {
    rt_frame_desc f;
    std::memset(&f, 0, sizeof(f));
    f.nx = nx; f.ny = ny; f.ns = ns; f.tile_rows = ny; f.tile_first = 0; f.tile_stride = 1;
    return f;
}
static const sample_window WHOLE = {false, 0, 0};
static cost_map_view no_map() { cost_map_view v = {}; v.scene_epoch_now = 5; v.opt_epoch_now = 9; return v; }
// the map a frame of this geometry and kernel_variant left, under the current epochs
static cost_map_view exact_map(const rt_frame_desc& f, const frame_geometry& g, int variant) {
    cost_map_view v = no_map();
    v.valid = true; v.has_total = true;
    v.key.nx = f.nx; v.key.ny = f.ny; v.key.tile_rows = f.tile_rows; v.key.tile_first = f.tile_first; v.key.tile_stride = f.tile_stride;
    v.key.local_rows = g.local_rows; v.key.kernel_variant = variant;
    v.scene_epoch = 5; v.opt_epoch = 9;
    return v;
}

static main_launch launch(const plan_facts& c, const rt_options& o, int kernel, size_t n_pixels, uint32_t work_items) {
    main_launch ml;
    const char* why = nullptr;
    CHECK(plan_main_launch(c, o, kernel, n_pixels, work_items, ml, why) == RT_OK && why == nullptr);
    return ml;
}
static frame_plan plan(const plan_facts& c, const rt_options& o, const rt_frame_desc& f, const frame_geometry& g, const cost_map_view& v,
                       const sample_window& w = WHOLE) {
    frame_plan p;
    const char* why = nullptr;
    CHECK(plan_frame(c, o, f, g, w, v, p, why) == RT_OK && why == nullptr);
    return p;
}
static bool same_sizes(const tier_sizes& a, int t1p, int t1f, int t1d, int hf, int sf, int sp, int wp) {
    return a.tier1_pixels == t1p && a.tier1_factor == t1f && a.tier1_depth == t1d && a.heavy_factor == hf && a.sparse_factor == sf &&
           a.sparse_percent == sp && a.work_percent == wp;
}
// a part's full record
static bool same_part(const frame_part& a, int begin, int end, part_rank on, bool fresh, bool reads, bool parks, bool writes, bool clear_before,
                      bool clear_after, unsigned grid, bool tiers, bool tail, int cost_begin) {
    return a.sample_begin == begin && a.sample_end == end && a.ranked_on == on && a.fresh == fresh && a.reads_state == reads &&
           a.parks_state == parks && a.writes_tile_cost == writes && a.clear_before == clear_before && a.clear_after == clear_after &&
           a.grid == grid && a.tiers == tiers && a.tail == tail && a.cost_begin == cost_begin;
}

static void check_main_launch() {
    const rt_options def;
    const uint32_t headline_items = 960000;   // 1200 x 800: 150 x 100 tiles of 64
    // ---- plan_main_launch, the auto LDS ladder: `image_bytes + sphere_bytes <= budget1` -> 2, `image_bytes <= budget1` -> 1, else 0
    {   main_launch ml = launch(scene(true, 158192), def, RT_KERNEL_STAGED, 960000, headline_items);   // 3 600 + 158 192 = 161 792
        CHECK(ml.lds_mode == 2 && ml.lds_bytes == 161792);
        ml = launch(scene(true, 158193), def, RT_KERNEL_STAGED, 960000, headline_items);               // one byte more: nodes only
        CHECK(ml.lds_mode == 1 && ml.lds_bytes == 3600);
        plan_facts c = scene(true, 1000);
        c.node_bytes = 161392;                                                                          // + the 400-byte prim table = 161 792
        ml = launch(c, def, RT_KERNEL_STAGED, 960000, headline_items);
        CHECK(ml.lds_mode == 1 && ml.lds_bytes == 161792);
        c.node_bytes = 161393;                                                                          // fits without the table, not with it
        ml = launch(c, def, RT_KERNEL_STAGED, 960000, headline_items);
        CHECK(ml.lds_mode == 0 && ml.lds_bytes == 0);
    }
    // ---- scan mode: `o.lds_mode < 0 && kernel == STAGED && scan_nodes > 0 && n_nodes <= scan_nodes` -> 4 (no LDS image)
    {   plan_facts c = scene(true);
        c.n_nodes = 24;                                                                                 // prim table (96 + 15) & ~15 = 96
        main_launch ml = launch(c, def, RT_KERNEL_STAGED, 4096, 4096);
        CHECK(ml.lds_mode == 4 && ml.lds_bytes == 0);
        c.n_nodes = 25;                                                                                 // table (100 + 15) & ~15 = 112
        ml = launch(c, def, RT_KERNEL_STAGED, 4096, 4096);
        CHECK(ml.lds_mode == 2 && ml.lds_bytes == 3200 + 112 + 16000);
        c.n_nodes = 24;
        rt_options o; o.lds_mode = 2;                                                                   // auto only
        ml = launch(c, o, RT_KERNEL_STAGED, 4096, 4096);
        CHECK(ml.lds_mode == 2 && ml.lds_bytes == 3200 + 96 + 16000);
        o = rt_options(); o.scan_nodes = 0;                                                             // 0 = never
        CHECK(launch(c, o, RT_KERNEL_STAGED, 4096, 4096).lds_mode == 2);
        CHECK(launch(c, def, RT_KERNEL_PIXEL, 4096, 4096).lds_mode == 0);                               // staged only
    }
    // ---- `lds_mode >= 3 && kernel != STAGED` -> 2; mode 3 on the staged kernel adds shade_bytes; the pixel kernel's mode 0
    {   rt_options o; o.lds_mode = 3;
        main_launch ml = launch(scene(true), o, RT_KERNEL_STAGED, 4096, 4096);
        CHECK(ml.lds_mode == 3 && ml.lds_bytes == 3600 + 16000 + 1000);
        ml = launch(scene(true), o, 2, 4096, 4096);                                                     // a kernel that is neither: no prim table
        CHECK(ml.lds_mode == 2 && ml.lds_bytes == 3200 + 16000);
        ml = launch(scene(true), o, RT_KERNEL_PIXEL, 4096, 4096);                                       // `kernel == PIXEL` -> 0
        CHECK(ml.lds_mode == 0 && ml.lds_bytes == 0);
        // ... and its grid: block 256, `ceil(work_items / 256)`, one resident workgroup
        CHECK(ml.block.x == 256 && ml.grid.x == 16 && ml.per_cu_resident == 1);
        ml = launch(scene(true), def, RT_KERNEL_PIXEL, 61 * 43, 3072);                                  // 61 x 43: 8 x 6 tiles
        CHECK(ml.grid.x == 12);
        ml = launch(scene(true), def, RT_KERNEL_PIXEL, 61 * 43, 3073);
        CHECK(ml.grid.x == 13);
    }
    // ---- the refusal: `lds_bytes > budget1`, text and status as rt_render reports them
    {   rt_options o; o.lds_mode = 3;
        plan_facts c = scene(true, 158192);                                                             // 161 792 + 1 000 of shade_bytes
        main_launch ml;
        const char* why = nullptr;
        CHECK(plan_main_launch(c, o, RT_KERNEL_STAGED, 4096, 4096, ml, why) == RT_ERR_INVALID);
        CHECK(why && std::strcmp(why, "requested lds_mode does not fit the CU's LDS") == 0);
        frame_plan p;
        why = nullptr;
        CHECK(plan_frame(c, o, frame(64, 64, 32), geometry(64, 64), WHOLE, no_map(), p, why) == RT_ERR_INVALID);
        CHECK(why && std::strcmp(why, "requested lds_mode does not fit the CU's LDS") == 0);
        o.lds_mode = 2;                                                                                 // exactly budget1 is not refused
        CHECK(plan_main_launch(c, o, RT_KERNEL_STAGED, 4096, 4096, ml, why) == RT_OK);
    }
    // ---- workgroup shapes: lean 2 x 512, the others 3 x 256; `grid = min(cu * per_cu, ceil(work_items / threads))`
    {   main_launch ml = launch(scene(true), def, RT_KERNEL_STAGED, 960000, headline_items);            // lds 19 600: fits 8 times
        CHECK(ml.block.x == 512 && ml.per_cu_resident == 2 && ml.grid.x == 512);                        // need 1 875
        ml = launch(scene(false), def, RT_KERNEL_STAGED, 960000, headline_items);
        CHECK(ml.block.x == 256 && ml.per_cu_resident == 3 && ml.grid.x == 768);                        // need 3 750
        ml = launch(scene(true), def, RT_KERNEL_STAGED, 4096, 4096);
        CHECK(ml.grid.x == 8 && ml.per_cu_resident == 2);                                               // need 8 < 512
        ml = launch(scene(true), def, RT_KERNEL_STAGED, 4097, 4097);
        CHECK(ml.grid.x == 9);
        // `lds_fit = lds_per_cu / (lds_bytes + 512)`; `lds_fit < per_cu` with neither option set: one workgroup of fam_max_threads
        ml = launch(scene(true, 77808), def, RT_KERNEL_STAGED, 960000, headline_items);                 // 2 x (81 408 + 512) = 163 840: fits twice
        CHECK(ml.block.x == 512 && ml.per_cu_resident == 2 && ml.grid.x == 512);
        ml = launch(scene(true, 77809), def, RT_KERNEL_STAGED, 960000, headline_items);                 // once: 1 x RT_LEAN_MAX_THREADS
        CHECK(ml.block.x == 512 && ml.per_cu_resident == 1 && ml.grid.x == 256);
        ml = launch(scene(false, 50501), def, RT_KERNEL_STAGED, 960000, headline_items);                // 3 x (54 101 + 512) = 163 839: fits 3 times
        CHECK(ml.block.x == 256 && ml.per_cu_resident == 3 && ml.grid.x == 768);
        ml = launch(scene(false, 50502), def, RT_KERNEL_STAGED, 960000, headline_items);                // twice: 1 x RT_HEAVY_MAX_THREADS
        CHECK(ml.block.x == 768 && ml.per_cu_resident == 1 && ml.grid.x == 256);
    }
    // ---- options wg_per_cu / threads and their clamps: threads to [64, family maximum], per_cu to lds_fit; no fall-back with an option set
    {   rt_options o; o.wg_per_cu = 4;
        main_launch ml = launch(scene(true), o, RT_KERNEL_STAGED, 960000, headline_items);
        CHECK(ml.per_cu_resident == 4 && ml.block.x == 512 && ml.grid.x == 1024);
        ml = launch(scene(true, 77809), o, RT_KERNEL_STAGED, 960000, headline_items);                   // lds_fit 1: clamped, threads stay
        CHECK(ml.per_cu_resident == 1 && ml.block.x == 512 && ml.grid.x == 256);
        ml = launch(scene(false, 50502), o, RT_KERNEL_STAGED, 960000, headline_items);                  // lds_fit 2; the others' threads stay 256
        CHECK(ml.per_cu_resident == 2 && ml.block.x == 256 && ml.grid.x == 512);
        o = rt_options(); o.threads = 32;
        ml = launch(scene(true), o, RT_KERNEL_STAGED, 960000, headline_items);
        CHECK(ml.block.x == 64 && ml.per_cu_resident == 2 && ml.grid.x == 512);
        o.threads = 1024;
        CHECK(launch(scene(true), o, RT_KERNEL_STAGED, 960000, headline_items).block.x == 512);
        CHECK(launch(scene(false), o, RT_KERNEL_STAGED, 960000, headline_items).block.x == 768);
        o.threads = 128;
        ml = launch(scene(false), o, RT_KERNEL_STAGED, 4096, 4096);
        CHECK(ml.block.x == 128 && ml.per_cu_resident == 3 && ml.grid.x == 32);
    }
    // ---- stage quorums: `latency_regime = STAGED && lean_family && pixels_per_lane < 2.75`; shade 16 : 32; newpath spheres-only 12 : 24, else 8
    {   // lean 2 x 512 on 256 CUs: 262 144 resident lanes, 2.75 of which are 720 896 pixels
        main_launch ml = launch(scene(true), def, RT_KERNEL_STAGED, 720896, headline_items);
        CHECK(ml.shade_threshold == 32 && ml.newpath_threshold == 24);
        ml = launch(scene(true), def, RT_KERNEL_STAGED, 720895, headline_items);
        CHECK(ml.shade_threshold == 16 && ml.newpath_threshold == 12);
        ml = launch(scene(true), def, RT_KERNEL_STAGED, 960000, headline_items);                        // the headline frame: 3.66 pixels per lane
        CHECK(ml.shade_threshold == 32 && ml.newpath_threshold == 24);
        ml = launch(scene(false), def, RT_KERNEL_STAGED, 100, 4096);                                    // the other families: never halved
        CHECK(ml.shade_threshold == 32 && ml.newpath_threshold == 8);
        ml = launch(scene(false), def, RT_KERNEL_STAGED, 960000, headline_items);
        CHECK(ml.shade_threshold == 32 && ml.newpath_threshold == 8);
        plan_facts c = scene(true);
        c.tex_level = 2;                                                                                // spheres only, not lean: 3 x 256
        ml = launch(c, def, RT_KERNEL_STAGED, 100, 4096);
        CHECK(ml.block.x == 256 && ml.shade_threshold == 32 && ml.newpath_threshold == 24);
        CHECK(launch(scene(true), def, RT_KERNEL_PIXEL, 100, 4096).shade_threshold == 32);              // staged only
        rt_options o; o.shade_threshold = 20; o.newpath_threshold = 10;                                 // the options win on both sides
        ml = launch(scene(true), o, RT_KERNEL_STAGED, 100, 4096);
        CHECK(ml.shade_threshold == 20 && ml.newpath_threshold == 10);
        ml = launch(scene(false), o, RT_KERNEL_STAGED, 960000, headline_items);
        CHECK(ml.shade_threshold == 20 && ml.newpath_threshold == 10);
    }
    // ---- kernel_variant: `kernel * 1000 + lds_mode * 100 + tex_level * 10 + spheres_only`
    {   plan_facts c = scene(true);
        CHECK(kernel_variant_of(c, launch(c, def, RT_KERNEL_STAGED, 4096, 4096)) == 3201);
        c = scene(false); c.tex_level = 2;
        CHECK(kernel_variant_of(c, launch(c, def, RT_KERNEL_STAGED, 4096, 4096)) == 3220);
        CHECK(kernel_variant_of(c, launch(c, def, RT_KERNEL_PIXEL, 4096, 4096)) == 20);
    }
}

static void check_tier_room() {
    const rt_options def;
    const rt_frame_desc f = frame(1200, 800, 32);
    const frame_geometry g = geometry(1200, 800);
    // ---- plan_tier_room: `fits` = tier data and `rt_tier_lds_bytes(leaves only) <= budget`; 25 slots are 25 * (64 * 32 + 32) = 52 000 bytes
    {   plan_facts c = scene(true);
        tier_room r = plan_tier_room(c, 52000);
        CHECK(r.fits && r.lds_scene == 1 && r.lds == 52000);                                            // (no spheres, materials or textures counted)
        CHECK(!plan_tier_room(c, 51999).fits);
        c.n_textures = 1;                                                                               // `lds_scene`: + 64 bytes fit too, or the leaves alone
        r = plan_tier_room(c, 52064);
        CHECK(r.fits && r.lds_scene == 1 && r.lds == 52064);
        r = plan_tier_room(c, 52063);
        CHECK(r.fits && r.lds_scene == 0 && r.lds == 52000);
        c.tier_data = false;
        CHECK(!plan_tier_room(c, 1 << 20).fits);
        // tail_grid = cu * min(by_lds, by_regs): `by_lds = lds_per_cu / (lds + 512)`, `by_regs = lean ? 4 : 3`
        CHECK(plan_tier_room(scene(true), 60000).tail_grid == 768);                                     // 163 840 / 52 512 = 3 < 4
        CHECK(plan_tier_room(scene(false), 60000).tail_grid == 768);                                    // 3 = 3
        c = scene(true); c.n_slots = 10;                                                                // 20 800 bytes: by_lds 7
        CHECK(plan_tier_room(c, 60000).tail_grid == 1024);
        c.spheres_only = false;
        CHECK(plan_tier_room(c, 60000).tail_grid == 768);
        c.n_slots = 30;                                                                                 // 62 400 bytes: by_lds 2, both families
        CHECK(plan_tier_room(c, 70000).tail_grid == 512);
        c.spheres_only = true;
        CHECK(plan_tier_room(c, 70000).tail_grid == 512);
        c.n_slots = 80;                                                                                 // 166 400 bytes: by_lds 0 -- the floor of 1
        CHECK(plan_tier_room(c, 1 << 20).tail_grid == 1);
    }
    // ---- plan_frame, lean budget: `lds_per_cu - per_cu * (lds_bytes + 512) - 1024`, or 0 where less than that is left
    {   frame_plan p = plan(scene(true), def, f, g, no_map());                                          // 163 840 - 2 * 20 112 - 1 024 = 122 592
        CHECK(p.room.fits && p.tier_possible && p.tier_waves_per_main_wg == 0);
        CHECK(p.tier_grid == 512);                                                                      // lean: `2 * num_cu`
        CHECK(p.tail_grid == 768 && p.room.lds == 52000 && p.room.lds_scene == 1);
        p = plan(scene(true, 51296), def, f, g, no_map());                                              // lds 54 896: 163 840 - 110 816 - 1 024 = 52 000
        CHECK(p.ml.per_cu_resident == 2 && p.room.fits && p.tier_possible && p.tail_grid == 768);
        p = plan(scene(true, 51297), def, f, g, no_map());                                              // 51 998 left
        CHECK(!p.room.fits && !p.tier_possible && p.tier_grid == 0 && p.tail_grid == 0);
        plan_facts c = scene(true, 77400);                                                              // lds 81 000: 2 * 81 512 + 1 024 > 163 840 -> 0
        c.n_slots = 1;
        p = plan(c, def, f, g, no_map());
        CHECK(p.ml.per_cu_resident == 2 && !p.room.fits && p.tail_grid == 0);
        c.n_slots = 0;                                                                                  // (an empty image fits a budget of 0)
        CHECK(plan(c, def, f, g, no_map()).room.fits);
    }
    // ---- other families: `budget = (lds_per_cu / per_cu - 1024) / tier_wgs_per_slot`, `tier_wgs_per_slot = max(block / 256, 1)`,
    // `tier_waves_per_main_wg = 4 * tier_wgs_per_slot`, `tier_grid = cu * per_cu * (waves / 4) / 2`
    {   frame_plan p = plan(scene(false), def, f, g, no_map());                                         // 3 x 256: 54 613 - 1 024 = 53 589
        CHECK(p.room.fits && p.tier_possible && p.tier_waves_per_main_wg == 4 && p.tier_grid == 384 && p.tail_grid == 768);
        plan_facts c = scene(false);
        c.n_slots = 25; c.n_textures = 24;                                                              // 52 000 + 1 536 = 53 536 <= 53 589
        CHECK(plan(c, def, f, g, no_map()).room.lds_scene == 1);
        c.n_textures = 25;                                                                              // 53 600: the leaves alone
        p = plan(c, def, f, g, no_map());
        CHECK(p.room.fits && p.room.lds_scene == 0 && p.room.lds == 52000);
        c = scene(false, 50502);                                                                        // 1 x 768: (163 840 - 1 024) / 3 = 54 272
        c.n_slots = 26;                                                                                 // 54 080
        p = plan(c, def, f, g, no_map());
        CHECK(p.ml.block.x == 768 && p.room.fits && p.tier_waves_per_main_wg == 12 && p.tier_grid == 384);   // 256 * 1 * 3 / 2
        c.n_slots = 27;                                                                                 // 56 160
        CHECK(!plan(c, def, f, g, no_map()).room.fits);
        rt_options o; o.threads = 128;                                                                  // 128 / 256 = 0 -> one tier workgroup a slot
        p = plan(scene(false), o, f, g, no_map());
        CHECK(p.tier_waves_per_main_wg == 4 && p.tier_grid == 384);
        c = scene(false); c.num_cu = 1;                                                                 // 1 * 1 * 1 / 2 = 0 -- the floor of 1
        o = rt_options(); o.wg_per_cu = 1;
        p = plan(c, o, f, g, no_map());
        CHECK(p.room.fits && p.tier_grid == 1 && p.tail_grid == 3);
    }
    // ---- `tier_possible = tier_kernel && lds_mode != 4 && tier1_pixels > 0`; the room is planned with `tier_kernel || handoff`;
    // `tail_grid = fits && handoff && (lds_mode != 4 || handoff_scan) ? room.tail_grid : 0`
    {   plan_facts scan = scene(true);
        scan.n_nodes = 24;
        frame_plan p = plan(scan, def, f, g, no_map());
        CHECK(p.ml.lds_mode == 4 && p.room.fits && !p.tier_possible && p.tail_grid == 768);
        rt_options o; o.handoff_scan = 0;
        CHECK(plan(scan, o, f, g, no_map()).tail_grid == 0);
        CHECK(plan(scene(true), o, f, g, no_map()).tail_grid == 768);                                   // (lds_mode 2: handoff_scan is not asked)
        o = rt_options(); o.tier_kernel = 0;
        p = plan(scene(true), o, f, g, no_map());
        CHECK(p.room.fits && !p.tier_possible && p.tail_grid == 768);                                   // room still planned for the tails
        o.handoff = 0;
        p = plan(scene(true), o, f, g, no_map());
        CHECK(!p.room.fits && !p.tier_possible && p.tail_grid == 0 && p.tier_grid == 0);
        o = rt_options(); o.handoff = 0;
        p = plan(scene(true), o, f, g, no_map());
        CHECK(p.room.fits && p.tier_possible && p.tier_grid == 512 && p.tail_grid == 0);
        o = rt_options(); o.tier1_pixels = 0;
        p = plan(scene(true), o, f, g, no_map());
        CHECK(p.room.fits && !p.tier_possible && p.tail_grid == 768);
        o = rt_options(); o.kernel = RT_KERNEL_PIXEL;                                                   // staged only
        CHECK(!plan(scene(true), o, f, g, no_map()).room.fits);
        plan_facts c = scene(true); c.tier_data = false;
        CHECK(!plan(c, def, f, g, no_map()).room.fits);
    }
}

static void check_tier_sizes() {
    const rt_options def;   // 1536, 45, 3, 20, 40, 35, 5
    const double above = 1.0000001;
    // ---- effective_tier_sizes, lean family: `> 2.75` the defaults, `> 1.375` the half's row, else the quarter's
    CHECK(same_sizes(effective_tier_sizes(2.75 * above, true, def), 1536, 45, 3, 20, 40, 35, 5));
    CHECK(same_sizes(effective_tier_sizes(2.75, true, def), 1536, 40, 3, 20, 40, 80, 5));
    CHECK(same_sizes(effective_tier_sizes(1.375 * above, true, def), 1536, 40, 3, 20, 40, 80, 5));
    CHECK(same_sizes(effective_tier_sizes(1.375, true, def), 8192, 20, 4, 15, 20, 80, 40));
    CHECK(same_sizes(effective_tier_sizes(0.6875 * above, true, def), 8192, 20, 4, 15, 20, 80, 40));
    CHECK(same_sizes(effective_tier_sizes(0.6875, true, def), 8192, 20, 4, 15, 20, 80, 40));
    // ---- other families: `> 2.75` 70 / 256 / 1; `> 1.375`; `> 0.6875` (work 20); else
    CHECK(same_sizes(effective_tier_sizes(2.75 * above, false, def), 256, 70, 1, 20, 40, 35, 5));
    CHECK(same_sizes(effective_tier_sizes(2.75, false, def), 4096, 30, 4, 20, 30, 80, 5));
    CHECK(same_sizes(effective_tier_sizes(1.375 * above, false, def), 4096, 30, 4, 20, 30, 80, 5));
    CHECK(same_sizes(effective_tier_sizes(1.375, false, def), 4096, 30, 4, 20, 30, 80, 20));
    CHECK(same_sizes(effective_tier_sizes(0.6875 * above, false, def), 4096, 30, 4, 20, 30, 80, 20));
    CHECK(same_sizes(effective_tier_sizes(0.6875, false, def), 8192, 20, 4, 15, 15, 80, 40));
    // ---- `tier_auto = 0`: the knobs as set, whatever the share; `sparse_factor >= heavy_factor`
    rt_options o; o.tier_auto = 0; o.tier1_pixels = 100; o.tier1_factor_x10 = 33; o.tier1_depth = 2; o.heavy_factor_x10 = 12; o.sparse_factor_x10 = 18;
    o.sparse_wg_percent = 50; o.sparse_work_percent = 7;
    for (double per_lane : {3.0, 2.0, 1.0, 0.5})
        for (bool lean : {true, false}) CHECK(same_sizes(effective_tier_sizes(per_lane, lean, o), 100, 33, 2, 12, 18, 50, 7));
    o.heavy_factor_x10 = 50;
    CHECK(same_sizes(effective_tier_sizes(3.0, true, o), 100, 33, 2, 50, 50, 50, 7));
    o = rt_options(); o.heavy_factor_x10 = 60;                                                          // (with tier_auto: whole lean frames keep the knobs)
    CHECK(same_sizes(effective_tier_sizes(3.0, true, o), 1536, 45, 3, 60, 60, 35, 5));
    // ---- plan_frame keys them by `n_pixels / (max_grid * block)`: the headline frame, 960 000 / 262 144 = 3.66, and its shares
    CHECK(same_sizes(plan(scene(true), def, frame(1200, 800, 32), geometry(1200, 800), no_map()).sizes, 1536, 45, 3, 20, 40, 35, 5));
    CHECK(same_sizes(plan(scene(true), def, frame(1200, 800, 32), geometry(1200, 400), no_map()).sizes, 1536, 40, 3, 20, 40, 80, 5));   // 1.83
    CHECK(same_sizes(plan(scene(true), def, frame(1200, 800, 32), geometry(1200, 200), no_map()).sizes, 8192, 20, 4, 15, 20, 80, 40));  // 0.92
    CHECK(same_sizes(plan(scene(false), def, frame(800, 800, 32), geometry(800, 800), no_map()).sizes, 256, 70, 1, 20, 40, 35, 5));     // 640 000 / 196 608 = 3.26
    CHECK(same_sizes(plan(scene(false), def, frame(800, 800, 32), geometry(800, 200), no_map()).sizes, 4096, 30, 4, 20, 30, 80, 20));   // 0.81
    CHECK(same_sizes(plan(scene(false), def, frame(800, 800, 32), geometry(800, 100), no_map()).sizes, 8192, 20, 4, 15, 15, 80, 40));   // 0.41
}

static void check_ranked() {
    const rt_options def;
    // ---- ranked: `lpt && kernel == STAGED && ns >= 2 * split_samples && n_tiles >= 64 && n_pixels < 2^31`, and no window
    const frame_geometry g = geometry(256, 256);
    CHECK(plan(scene(true), def, frame(256, 256, 32), g, no_map()).ranked);
    CHECK(!plan(scene(true), def, frame(256, 256, 31), g, no_map()).ranked);                            // 2 * 16 - 1
    rt_options o; o.lpt = 0;
    CHECK(!plan(scene(true), o, frame(256, 256, 32), g, no_map()).ranked);
    o = rt_options(); o.kernel = RT_KERNEL_PIXEL;
    CHECK(!plan(scene(true), o, frame(256, 256, 32), g, no_map()).ranked);
    o = rt_options(); o.split_samples = 20;
    CHECK(!plan(scene(true), o, frame(256, 256, 39), g, no_map()).ranked);
    CHECK(plan(scene(true), o, frame(256, 256, 40), g, no_map()).ranked);
    CHECK(plan(scene(true), def, frame(64, 64, 32), geometry(64, 64), no_map()).ranked);                // 8 x 8 = 64 tiles
    CHECK(!plan(scene(true), def, frame(72, 56, 32), geometry(72, 56), no_map()).ranked);               // 9 x 7 = 63
    // an unranked frame is one part on the plain grid, no state, no tail, nothing to grow
    frame_plan p = plan(scene(true), def, frame(256, 256, 31), g, no_map());
    CHECK(p.n_parts == 1 && same_part(p.parts[0], 0, 31, RANK_NONE, false, false, false, false, false, false, 128, false, false, 0));
    CHECK(p.handoff_capacity == 0 && !p.tail_ordered && p.order_min == 0 && p.order_max == 0 && !p.cost_out && !p.map_usable);
    CHECK(p.ranked_tiles == 0 && p.ranked_pixels == 0 && p.cost_map_pixels == 0 && p.handoff_ordered_capacity == 0 && p.handoff_scratch_words == 0);
    CHECK(p.tail_grid == 768);                                                                          // (planned, not used)
    // a progressive window: the staged kernel whatever the option says, one unranked part resumed from (not the first) and parked into the state
    o = rt_options(); o.kernel = RT_KERNEL_PIXEL;
    const sample_window first = {true, 0, 40}, later = {true, 40, 100};
    p = plan(scene(true), o, frame(256, 256, 1), g, exact_map(frame(256, 256, 1), g, 3201), first);
    CHECK(p.kernel == RT_KERNEL_STAGED && !p.ranked && p.n_parts == 1);
    CHECK(same_part(p.parts[0], 0, 40, RANK_NONE, false, false, true, false, false, false, 128, false, false, 0));
    p = plan(scene(true), o, frame(256, 256, 1), g, no_map(), later);
    // (cost_begin: `(state_in && !fresh) ? 0 : sample_begin` -- a resumed part's parked costs count from sample 0)
    CHECK(!p.ranked && p.n_parts == 1 && same_part(p.parts[0], 40, 100, RANK_NONE, false, true, true, false, false, false, 128, false, false, 0));
}

static void check_handoff() {
    const rt_options def;
    const rt_frame_desc f = frame(1200, 800, 32);
    const frame_geometry g = geometry(1200, 800);
    // ---- the headline frame: 1200 x 800, lean, 2 x 512 threads, a tail of 768 workgroups = 3 072 waves
    frame_plan p = plan(scene(true), def, f, g, no_map());
    CHECK(p.ml.block.x == 512 && p.ml.per_cu_resident == 2 && p.tail_grid == 768);
    CHECK(p.handoff_pixels == 36864);                                                                   // `handoff_order && lean ? 12 : 6` per wave
    CHECK(p.handoff_capacity == 262144);                                                                // `cu * per_cu * threads`
    CHECK(p.handoff_poll_ticks == 100000);                                                              // `handoff_poll_us * 100`
    CHECK(p.tail_ordered && p.order_min == 6144 && p.order_max == 98304);                               // 2 and 32 per wave
    CHECK(p.handoff_ordered_capacity == 262144 && p.handoff_scratch_words == 257 * (384 + 1));          // 98 304 / 256 workgroups + 1, of 257 buckets
    rt_options o; o.handoff_order = 0;
    p = plan(scene(true), o, f, g, no_map());
    CHECK(p.handoff_pixels == 18432 && p.handoff_capacity == 262144);                                   // six per wave in push order
    CHECK(!p.tail_ordered && p.order_min == 0 && p.order_max == 0 && p.handoff_ordered_capacity == 0 && p.handoff_scratch_words == 0);
    p = plan(scene(false), def, f, g, no_map());                                                        // the other families stay at 6
    CHECK(p.tail_grid == 768 && p.handoff_pixels == 18432 && p.handoff_capacity == 196608 && p.tail_ordered);
    // ---- the `n_pixels / 8` cap, an explicit handoff_pixels
    p = plan(scene(true), def, frame(256, 256, 32), geometry(256, 256), no_map());
    CHECK(p.handoff_pixels == 8192);
    p = plan(scene(true), def, frame(1200, 800, 32), geometry(1200, 245), no_map());                    // 294 000 / 8 = 36 750 < 36 864
    CHECK(p.handoff_pixels == 36750);
    p = plan(scene(true), def, frame(1200, 800, 32), geometry(1200, 246), no_map());                    // 36 900
    CHECK(p.handoff_pixels == 36864);
    o = rt_options(); o.handoff_pixels = 100;
    CHECK(plan(scene(true), o, f, g, no_map()).handoff_pixels == 100);
    o.handoff_pixels = 0;
    CHECK(plan(scene(true), o, f, g, no_map()).handoff_pixels == 0);
    // ---- `order_max = min(32 * tail_waves, capacity)`; the capacity is what the scene's queue already holds where that is more
    o = rt_options(); o.wg_per_cu = 1; o.threads = 64;
    p = plan(scene(true), o, f, g, no_map());
    CHECK(p.handoff_capacity == 16384 && p.order_min == 6144 && p.order_max == 16384 && p.handoff_scratch_words == 257 * (64 + 1));
    plan_facts c = scene(true);
    c.handoff_capacity = 20000;
    p = plan(c, o, f, g, no_map());
    CHECK(p.handoff_capacity == 20000 && p.order_max == 20000 && p.handoff_ordered_capacity == 20000);
    CHECK(plan(c, def, f, g, no_map()).handoff_capacity == 262144);
    // ---- no hand-off: option handoff 0, or a tier image that does not fit
    o = rt_options(); o.handoff = 0;
    p = plan(scene(true), o, f, g, no_map());
    CHECK(p.ranked && p.handoff_capacity == 0 && !p.tail_ordered && !p.parts[0].tail && !p.parts[1].tail);
}

static void check_parts() {
    const rt_options def;
    const rt_frame_desc f = frame(64, 64, 64);
    const frame_geometry g = geometry(64, 64);   // 4 096 work items: 8 lean workgroups
    // a ranked part's grid, lean, an eighth-like share (0.016 pixels per lane: sparse_percent 80): `normal_need + max_grid * 80 / 100` = 8 + 409
    const unsigned RG = 417;
    // ---- an exact map: one fresh part ranked on the map, one clear, cost_out
    frame_plan p = plan(scene(true), def, f, g, exact_map(f, g, 3201));
    CHECK(p.ranked && p.map_usable && p.map_exact && p.cost_out && p.n_parts == 1 && p.ranked_parts == 1);
    CHECK(same_part(p.parts[0], 0, 64, RANK_MAP, true, true, false, false, true, false, RG, true, true, 0));
    CHECK(p.max_grid == 512 && p.normal_need == 8 && p.sparse_stride == 8 && p.semi_stride == 1 && p.smooth_percent == 0);
    CHECK(p.ranked_tiles == 64 && p.ranked_pixels == 4096 && p.cost_map_pixels == 4096);
    CHECK(p.key.nx == 64 && p.key.ny == 64 && p.key.tile_rows == 64 && p.key.tile_first == 0 && p.key.tile_stride == 1 && p.key.local_rows == 64 &&
          p.key.kernel_variant == 3201);
    // ---- a stale map (either epoch has moved): part 1 ranked on the map prior, the second clear behind its ranking, the last part on measured rays
    for (int which = 0; which < 2; ++which) {
        cost_map_view v = exact_map(f, g, 3201);
        (which ? v.opt_epoch : v.scene_epoch) -= 1;
        p = plan(scene(true), def, f, g, v);
        CHECK(p.map_usable && !p.map_exact && p.cost_out && p.n_parts == 2 && p.ranked_parts == 2);
        CHECK(same_part(p.parts[0], 0, 16, RANK_MAP, true, true, true, true, true, true, RG, true, true, 0));
        CHECK(same_part(p.parts[1], 16, 64, RANK_MEASURED, false, true, false, false, false, false, RG, true, true, 0));
    }
    // ---- a map of no use: another view, another kernel variant, not valid, a total of 0 -> the calibration prior ranks part 1
    for (int which = 0; which < 5; ++which) {
        cost_map_view v = exact_map(f, g, 3201);
        if (which == 0) v = no_map();
        if (which == 1) v.key.local_rows = 56;
        if (which == 2) v.key.kernel_variant = 3101;
        if (which == 3) v.valid = false;
        if (which == 4) v.has_total = false;
        p = plan(scene(true), def, f, g, v);
        CHECK(!p.map_usable && !p.map_exact && p.cost_out && p.n_parts == 2);
        CHECK(same_part(p.parts[0], 0, 16, RANK_CALIBRATION, true, true, true, true, true, true, RG, true, true, 0));
        CHECK(same_part(p.parts[1], 16, 64, RANK_MEASURED, false, true, false, false, false, false, RG, true, true, 0));
    }
    // ---- `prior = 0`, or no calibration and no map: part 1 unranked on the plain grid (8 workgroups), the first clear only
    {   rt_options o; o.prior = 0;
        p = plan(scene(true), o, f, g, exact_map(f, g, 3201));                                          // (prior 0: the map is not read either)
        CHECK(!p.map_usable && p.n_parts == 2 && p.ranked_parts == 2);
        CHECK(same_part(p.parts[0], 0, 16, RANK_NONE, false, false, true, true, true, false, 8, false, true, 0));
        CHECK(same_part(p.parts[1], 16, 64, RANK_MEASURED, false, true, false, false, false, false, RG, true, true, 0));
        plan_facts c = scene(true); c.calibrated = false;
        p = plan(c, def, f, g, no_map());
        CHECK(same_part(p.parts[0], 0, 16, RANK_NONE, false, false, true, true, true, false, 8, false, true, 0));
        p = plan(c, def, f, g, exact_map(f, g, 3201));                                                  // (the map needs no calibration)
        CHECK(p.n_parts == 1 && p.parts[0].ranked_on == RANK_MAP);
    }
    // ---- presplit_samples: part 1b = [presplit, split) ranked on measured rays, resumed and parked
    {   rt_options o; o.presplit_samples = 8;
        p = plan(scene(true), o, f, g, no_map());
        CHECK(p.n_parts == 3 && p.ranked_parts == 3);
        CHECK(same_part(p.parts[0], 0, 8, RANK_CALIBRATION, true, true, true, true, true, true, RG, true, true, 0));
        CHECK(same_part(p.parts[1], 8, 16, RANK_MEASURED, false, true, true, true, false, false, RG, true, true, 0));
        CHECK(same_part(p.parts[2], 16, 64, RANK_MEASURED, false, true, false, false, false, false, RG, true, true, 0));
        o.presplit_samples = 16;                                                                        // `presplit < split` only
        CHECK(plan(scene(true), o, f, g, no_map()).n_parts == 2);
        // ---- resplit_samples: part 1c = [split, resplit) where `resplit > split && ns >= 2 * resplit`
        o = rt_options(); o.resplit_samples = 32;
        p = plan(scene(true), o, f, g, no_map());                                                       // ns 64 = 2 * 32
        CHECK(p.n_parts == 3);
        CHECK(same_part(p.parts[0], 0, 16, RANK_CALIBRATION, true, true, true, true, true, true, RG, true, true, 0));
        CHECK(same_part(p.parts[1], 16, 32, RANK_MEASURED, false, true, true, true, false, false, RG, true, true, 0));
        CHECK(same_part(p.parts[2], 32, 64, RANK_MEASURED, false, true, false, false, false, false, RG, true, true, 0));
        p = plan(scene(true), o, frame(64, 64, 63), g, no_map());
        CHECK(p.n_parts == 2 && same_part(p.parts[1], 16, 63, RANK_MEASURED, false, true, false, false, false, false, RG, true, true, 0));
        o.resplit_samples = 16;
        CHECK(plan(scene(true), o, f, g, no_map()).n_parts == 2);
        o.resplit_samples = 32; o.presplit_samples = 8;                                                 // all four
        p = plan(scene(true), o, f, g, exact_map(f, g, 3201));                                          // (an exact map still makes it one)
        CHECK(p.n_parts == 1);
        p = plan(scene(true), o, f, g, no_map());
        CHECK(p.n_parts == 4 && p.parts[3].sample_begin == 32 && p.parts[3].sample_end == 64 && p.parts[2].sample_begin == 16);
    }
    // ---- `cost_map = 0`: no cost_out, no map buffer, the map not read
    {   rt_options o; o.cost_map = 0;
        p = plan(scene(true), o, f, g, exact_map(f, g, 3201));
        CHECK(p.ranked && !p.cost_out && p.cost_map_pixels == 0 && !p.map_usable && p.n_parts == 2 && p.parts[0].ranked_on == RANK_CALIBRATION);
    }
    // ---- `map_read = lean_family || !tier_possible`: not read where tier workgroups take main slots, written all the same
    {   const unsigned RH = 768;   // `tier_waves_per_main_wg > 0 && tier_possible`: the whole resident grid, 256 * 3
        p = plan(scene(false), def, f, g, exact_map(f, g, 3200));
        CHECK(p.tier_possible && !p.map_usable && p.cost_out && p.n_parts == 2 && p.semi_stride == 0);
        CHECK(same_part(p.parts[0], 0, 16, RANK_CALIBRATION, true, true, true, true, true, true, RH, true, true, 0));
        CHECK(same_part(p.parts[1], 16, 64, RANK_MEASURED, false, true, false, false, false, false, RH, true, true, 0));
        rt_options o; o.tier_kernel = 0;   // 3 x 256, 16 workgroups needed + 768 * 80 / 100 sparse = 630; no tier 1 beside any part
        p = plan(scene(false), o, f, g, exact_map(f, g, 3200));
        CHECK(!p.tier_possible && p.map_exact && p.n_parts == 1);
        CHECK(same_part(p.parts[0], 0, 64, RANK_MAP, true, true, false, false, true, false, 630, false, true, 0));
    }
    // ---- the ranked grid's other terms: no sparse workgroups with `sparse_stride = 0`; the clamp to max_grid (the headline: 1 875 + 179 > 512)
    {   rt_options o; o.sparse_stride = 0; o.semi_stride = 0; o.cost_smooth_percent = 30;
        p = plan(scene(true), o, f, g, no_map());
        CHECK(p.parts[0].grid == 8 && p.parts[1].grid == 8 && p.sparse_stride == 0 && p.semi_stride == 0 && p.smooth_percent == 30);
        p = plan(scene(true), def, frame(1200, 800, 32), geometry(1200, 800), no_map());
        CHECK(p.normal_need == 1875 && p.parts[0].grid == 512 && p.parts[1].grid == 512 && p.parts[1].sample_end == 32);
    }
}

static void check_adaptive() {
    // ---- rt_render_adaptive's crossover: `active <= (lean ? 32 : 6) * tail_waves`, with adaptive_tier 0 = never and 1 = wherever the image fits
    const rt_options def;
    const plan_facts lean = scene(true), other = scene(false);
    const tier_room room = plan_tier_room(lean, lean.lds_per_cu - 2048);
    CHECK(room.fits && room.tail_grid == 768);                                                          // 3 072 waves
    CHECK(adaptive_use_tier(lean, room, def, 98304) && !adaptive_use_tier(lean, room, def, 98305));     // 32 * 3 072
    CHECK(adaptive_use_tier(other, room, def, 18432) && !adaptive_use_tier(other, room, def, 18433));   // 6 * 3 072
    rt_options o; o.adaptive_tier = 0;
    CHECK(!adaptive_use_tier(lean, room, o, 1) && !adaptive_use_tier(other, room, o, 1));
    o.adaptive_tier = 1;
    CHECK(adaptive_use_tier(lean, room, o, 4000000) && adaptive_use_tier(other, room, o, 4000000));
    const tier_room none = {false, 0, 0, 0};
    CHECK(!adaptive_use_tier(lean, none, o, 1) && !adaptive_use_tier(lean, none, def, 1));
}

int main() {
    check_main_launch();
    check_tier_room();
    check_tier_sizes();
    check_ranked();
    check_handoff();
    check_parts();
    check_adaptive();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("frame plan ok\n");
    return 0;
}
