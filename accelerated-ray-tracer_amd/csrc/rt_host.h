// rt_host.h -- the host internals of librt_mi355x.so, declared once for its host translation units: rt_abi.hip (which defines
// the globals), rt_abi_debug.hip (the rt_debug_* seams) and rt_multi.hip.  The device table, the options, the error state and
// its macros, the memory of one call, struct rt_scene and rt_progressive, the frame checks.  Everything but the two structs the
// C ABI names lives in namespace rt_host, so the library's rt_* C symbols are include/rt_abi.h's and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt_abi.h"
#include "rt_call_buffers.h"
#include "rt_device.h"
#include "rt_frame_plan.h"
#include "rt_owned.h"
#include "rt_refit_host.h"

namespace rt_host {

// Devices this process has initialised (rt_init / rt_init_devices).  A scene remembers the device it was created on and
// every entry point that touches it makes that device current first, so a caller may drive several devices from one
// thread (rt_multi_*) or change the current device between calls.
struct device_info {
    bool ready = false;
    int num_cu = 256;
    size_t lds_per_cu = 160 * 1024;
};
enum { RT_MAX_DEVICES = 16 };
extern device_info g_devices[RT_MAX_DEVICES];
extern int g_device;              // device new scenes are created on (the last rt_init)
extern int g_last_hip_error;
extern std::string g_detail;

extern rt_options g_opt;   // the tuning knobs (rt_set_option; struct rt_options: rt_frame_plan.h)
// bumped by every rt_set_option / rt_reset_options call: a cost map recorded under another value counts as stale (struct rt_scene)
extern unsigned long long g_opt_epoch;

// the reference's checkCudaErrors (main.cu:23-35) records "<code> at file:line 'expr'"; it then
// exits with 99, which a library must not do, so the status is returned instead.
inline rt_status hip_failed(hipError_t e, const char* file, int line, const char* expr) {
    g_last_hip_error = (int)e;
    char buf[512];
    snprintf(buf, sizeof(buf), "HIP error = %u at %s:%d '%s' (%s)", (unsigned)e, file, line, expr, hipGetErrorString(e));
    g_detail = buf;
    return RT_ERR_HIP;
}
#define HIPCHK(expr) do { const hipError_t e_ = (hipError_t)(expr); if (e_ != hipSuccess) return rt_host::hip_failed(e_, __FILE__, __LINE__, #expr); } while (0)
// a step that returns an rt_status: a failure is the caller's result
#define RT_TRY(expr) do { const rt_status st_ = (expr); if (st_ != RT_OK) return st_; } while (0)

inline rt_status invalid(const char* why) { g_detail = why; return RT_ERR_INVALID; }

rt_status init_device(int device_ordinal);
// makes the scene's device current (a no-op when it already is)
inline rt_status use_device(int device) {
    if (device < 0 || device >= RT_MAX_DEVICES || !g_devices[device].ready) { g_detail = "rt_init has not succeeded for this device"; return RT_ERR_NO_DEVICE; }
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != device) HIPCHK(hipSetDevice(device));
    return RT_OK;
}

// 8x8 pixel tiles across `pixels` pixels or rows (the tile grid of a call is tiles_across(nx) x tiles_across(local_rows))
inline int tiles_across(int pixels) { return (pixels + 7) / 8; }

// A device copy of `bytes` bytes in an allocation of its own (`to`), zero-filled up to the next multiple of 64 bytes.
inline rt_status upload(const void* src, size_t bytes, owned<char>& to) {
    // always allocate something so kernels never see a null array base
    const size_t room = ((bytes ? bytes : 1) + 63) & ~(size_t)63;
    HIPCHK(to.grow(room));
    hipError_t e = hipMemset(to, 0, room);
    if (e == hipSuccess && bytes) e = hipMemcpy(to, src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { to.adopt(nullptr, 0); HIPCHK(e); }
    return RT_OK;
}

// Device memory of one call, freed when the call returns: allocations of their own (get), which a caller may cut into
// 256-byte-rounded pieces (rounded, take: rt_call_buffers.h).  A call that enqueues work on the memory guards it with its stream:
// every way out but the one through settled() -- the call has waited for its work, or leaves it to the caller's stream (finish)
// -- synchronises that stream before the memory is freed.
struct call_memory : call_pieces {
    std::vector<owned<char>> all;
    hipStream_t stream = nullptr;
    bool guarded = false;
    ~call_memory() { if (guarded && !all.empty()) (void)hipStreamSynchronize(stream); }   // nothing of a failed call may still use the memory (freed next)
    void guard(hipStream_t st) { stream = st; guarded = true; }
    void settled() { guarded = false; }
    hipError_t get(void** p, size_t bytes) {
        owned<char> b;
        const hipError_t e = (hipError_t)b.grow(bytes ? bytes : 1);
        if (e == hipSuccess) { *p = b.get(); all.push_back(std::move(b)); }
        return e;
    }
    rt_status finish(bool wait) { if (wait) HIPCHK(hipStreamSynchronize(stream)); settled(); return RT_OK; }
};

}  // namespace rt_host

struct rt_scene {
    int device = 0;             // the device every allocation below lives on: current when the scene is deleted (rt_scene_destroy)
    rt_scene_dev dev;
    std::vector<owned<char>> allocs;   // the scene's arrays (upload_arrays)
    bool spheres_only = false, need_uv = false;
    int tex_level = 0;
    size_t node_bytes = 0, sphere_bytes = 0, shade_bytes = 0;   // node_bytes: the walk array; shade_bytes: materials + textures
    double walk_tests_before = 0, walk_tests_after = 0;          // expected box tests per calibration ray, reference tree / walk array
    // per-frame resources, each grown where a frame needs more than it holds
    owned<unsigned long long> d_ray_counter;
    owned<unsigned int> d_work_counter;
    owned<float> d_fb;
    owned<unsigned int> d_tile_cost;   // cost prepass: rays per 8x8 tile
    owned<unsigned int> d_tile_order;  // tiles in descending cost
    owned<rt_pixel_state> d_state;     // split frames: pixels parked between the two parts
    owned<unsigned long long> d_heavy_list;   // (cost << 32 | pixel), unsorted, from rt_collect_heavy_kernel
    owned<unsigned int> d_heavy_pixels;       // heavy pixels, dearest first
    owned<unsigned long long> d_handoff;      // tail hand-off queue: (sample << 32 | pixel), one entry per resident lane at most
    owned<unsigned long long> d_handoff_ordered;   // ... ordered for the tail launch (rt_handoff_order.h), grown like d_handoff
    owned<unsigned int> d_handoff_scratch;          // ... the ordering kernels' bucket counts
    owned<rt_rank_info> d_rank;               // tier sizes of the next ranked launch (written and read on the device only)
    owned<unsigned int> d_cal_cost;           // cost prior: rays per pixel of the calibration frame (cal_nx x cal_ny at 4 spp)
    int cal_nx = 0, cal_ny = 0;
    // The cost map: the rays every local pixel cost over all its samples, written by the last launches of the last ranked frame
    // (rt_frame_params::cost_out) and valid once rt_frame_finish has closed that frame.  A pixel's cost depends on the scene, the
    // camera, the frame geometry and the row partition -- `key` and `scene_epoch` -- and not on the seed or the sample count.
    // Rendering the same view again (key and both epochs equal: the map is EXACT) therefore needs no first look: the frame is
    // ranked on the map and runs as one part.  After rt_scene_set_camera / rt_scene_update_spheres without recalibration, or any
    // option call, the map is STALE: it replaces the calibration frame as the prior of part 1.  Scheduling only.
    struct cost_map_state {
        owned<unsigned int> d;                    // one word per local pixel, grown like the ranked buffers (grow: the map is lost)
        bool valid = false, pending = false;      // pending: the frame in flight writes it
        cost_map_key key, last_key;               // of the map; of the last ranked frame (rt_debug_set_cost_map)
        bool have_last_key = false;
        unsigned long long scene_epoch = 0, opt_epoch = 0, total = 0;   // of the map; total = the sum of its words (0: not used)
        rt_status grow(size_t pixels) { if (d.capacity() < pixels) valid = false; HIPCHK(d.grow(pixels)); return RT_OK; }
    } cost_map;
    unsigned long long scene_epoch = 0;           // bumped when the camera or a sphere changes
    hipStream_t tier_stream = nullptr;            // the tier kernel's stream (forked from / joined to the caller's stream by events)
    hipEvent_t ev_fork[4] = {nullptr, nullptr, nullptr, nullptr}, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
    frame_plan plan;                              // of the last frame render_impl enqueued (rt_frame_finish and the debug entries read it)
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool frame_pending = false;
    hipStream_t pending_stream = nullptr;
    rt_stats pending_stats;
    // rt_render_adaptive (cached like d_state): parked pixels, the average at the previous checkpoint, two pixel lists, the tail
    // queue, and a small block: [0] the decision kernel's append head, then an rt_rank_info and the host copy of a work-counter block
    owned<rt_pixel_state> d_adapt_state;
    owned<float> d_adapt_half;
    owned<uint32_t> d_adapt_list[2];
    owned<unsigned long long> d_adapt_queue;
    owned<int32_t> d_adapt_spp;                  // host spp_out: the device map copied back
    owned<uint32_t> d_adapt_count;
    owned<rt_rank_info> d_adapt_rank;
    std::vector<hipEvent_t> adapt_events;        // two per pass (rt_debug_adaptive_passes)
    std::vector<long long> adapt_log;            // per pass of the last adaptive frame: route, active pixels, sample_begin, sample_end
    std::vector<float> adapt_ms;
    rt_rank_info adapt_rank_host;                // host sides of the small copies between passes (alive until the next sync)
    unsigned int adapt_wc_host[RT_WORK_COUNTER_BYTES / 4];
    // rt_render_variance: per local pixel T_{b-1}, A, Q, three doubles (the parked pixels live in d_adapt_state, a host
    // variance_out's device image in d_adapt_spp: 4 bytes per pixel either way)
    owned<double> d_var_acc;
    // rt_scene_update_spheres, _instances and _quads: the lookup tables of the refit kernels, built on
    // the scene's first update from a read-back of the node arrays, so that a scene that never moves pays nothing; refit.block
    // holds all of them
    int32_t n_instances = 0, n_media = 0;        // of the description (rt_scene_dev carries neither)
    int32_t n_quads = 0, n_boxes = 0;
    struct refit_tables {
        bool ready = false;
        owned<char> block;                       // one allocation, cut into the arrays of `p` and the stamps
        rt_refit_params p;                       // the per-scene half of the kernels' argument, filled once
        std::vector<char> instanced;             // per sphere: the child of an instance (kept from rt_scene_create, host only)
        std::vector<int32_t> inst_child;         // per instance: its child, which no update changes (the same)
        uint32_t* stamp[rt_refit::KINDS] = {};   // per kind (the kinds index different arrays): one word per record ...
        uint32_t epoch[rt_refit::KINDS] = {};    // ... equal to this after the update that last replaced the record
        owned<int32_t> d_indices;                // the update's index list and (host records, in bytes) its records on the device
        owned<char> d_records;
    } refit;
};

// Progressive accumulation (rt_render_window): the parked pixels of one frame description between windows.
struct rt_progressive {
    rt_scene* scene = nullptr;
    owned<rt_pixel_state> d_state;
    size_t pixels = 0;
    rt_frame_desc frame;         // the description it was made for (its partition must not change between windows)
    int32_t next_sample = 0;     // the sample_begin the next window must have
};

namespace rt_host {

// Validate; derive the host arrays (rt_scene_plan.h); upload; create the per-frame resources; build the tier data; build the walk.
rt_status rt_internal_scene_create_on(int device, const rt_scene_desc* d, rt_scene** out);
// init_device, and the device new scenes are created on from then on (rt_init)
rt_status rt_internal_init_device(int device_ordinal);

// The words of the four failed checks.  They differ between the entry points, and tests and the Python layer match on them.
struct frame_texts { const char *size, *large, *partition, *tiles; };
const frame_texts RENDER_FRAME_TEXTS = {"nx, ny and ns must be positive", "frame too large", "bad row partition", "frame too large"};
const frame_texts STATE_FRAME_TEXTS = {"bad frame size", "bad frame size", "bad row partition", "bad frame size"};

// The frame checks of every entry point that takes a frame: a positive size (and sample count, where the entry point reads
// f->ns), fewer than 2^31 pixels, a valid row partition, fewer than 2^31 work items.  `who` (may be null) prefixes the text of
// a failed check.  No HIP call.
inline rt_status check_frame(const char* who, const rt_frame_desc* f, bool check_ns, const frame_texts& text, frame_geometry& g) {
    auto bad = [&](const char* why) { return who ? invalid((std::string(who) + ": " + why).c_str()) : invalid(why); };
    if (f->nx <= 0 || f->ny <= 0 || (check_ns && f->ns <= 0)) return bad(text.size);
    if ((long long)f->nx * f->ny >= (1ll << 31)) return bad(text.large);
    g.local_rows = rt_frame_local_rows(f);
    if (g.local_rows < 0) return bad(text.partition);
    g.tiles_x = tiles_across(f->nx); g.tiles_y = tiles_across(g.local_rows);
    if ((long long)g.tiles_x * g.tiles_y * 64 >= (1ll << 31)) return bad(text.tiles);
    g.n_pixels = (size_t)g.local_rows * (size_t)f->nx;
    g.work_items = (uint32_t)g.tiles_x * (uint32_t)g.tiles_y * 64u;
    return RT_OK;
}

// What the plans of rt_frame_plan.h read of the scene and its device.
inline plan_facts plan_facts_of(const rt_scene* s) {
    const device_info& d = g_devices[s->device];
    plan_facts c;
    c.num_cu = d.num_cu; c.lds_per_cu = d.lds_per_cu;
    c.spheres_only = s->spheres_only; c.tex_level = s->tex_level;
    c.node_bytes = s->node_bytes; c.sphere_bytes = s->sphere_bytes; c.shade_bytes = s->shade_bytes; c.n_nodes = s->dev.n_nodes;
    c.tier_data = s->dev.leaf_lo != nullptr;
    c.n_slots = s->dev.n_slots; c.n_spheres = s->dev.n_spheres; c.n_materials = s->dev.n_materials; c.n_textures = s->dev.n_textures;
    c.calibrated = s->d_cal_cost && s->cal_nx > 0 && s->cal_ny > 0;
    c.handoff_capacity = s->d_handoff.capacity();
    return c;
}

}  // namespace rt_host
