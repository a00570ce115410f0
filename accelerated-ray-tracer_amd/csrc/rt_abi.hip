// rt_abi.hip -- implementation of include/rt_abi.h: device bookkeeping, scene
// creation (what it uploads is decided in rt_scene_plan.h: the checks, the walk-array
// planner, the regrouped hierarchies, the tier data; here: the uploads, the
// calibration pass and the cost prior), frame launch (rt_frame_plan.h decides,
// this file enqueues), statistics.  The kernels are in rt_kernel_pixel.hip, rt_staged_*.hip
// (rt_kernel_staged.h), rt_tier_*.hip (rt_kernel_tier.h), rt_rank.hip and, for
// rt_scene_update_spheres, rt_kernel_refit.hip (host half: rt_refit_host.h).  The rt_debug_* entries are in rt_abi_debug.hip;
// what this file shares with it and with rt_multi.hip -- the globals defined below, struct rt_scene -- is declared in rt_host.h.
// There is no CPU render path here or anywhere else in the
// library: without a HIP device every entry point fails with
// RT_ERR_NO_DEVICE / RT_ERR_HIP.
#include <algorithm>
#include <cfloat>
#include <utility>
#include <cmath>
#include <functional>

#include "rt_host.h"
#include "rt_handoff_order.h"
#include "rt_scene_plan.h"

namespace rt_host {
device_info g_devices[RT_MAX_DEVICES];
int g_device = -1;
int g_last_hip_error = 0;
std::string g_detail;
rt_options g_opt;
unsigned long long g_opt_epoch = 0;
}  // namespace rt_host
using namespace rt_host;

namespace {

// One row of an upload table: `count` elements at `src` go to the device, where *dst points at them afterwards.
struct array_upload { const void* src; size_t bytes; const void** dst; };
template <class T> array_upload array_of(const T* src, size_t count, const T** dst) { return {src, count * sizeof(T), (const void**)dst}; }
template <class T> array_upload array_of(const std::vector<T>& v, const T** dst) { return array_of(v.data(), v.size(), dst); }

// picks the kernel family; LDS_MODE and texture level select the instantiation inside (rt_staged_*.hip)
hipError_t launch_render(int kernel, int lds_mode, const rt_scene* s, const rt_frame_params& fp, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream) {
    if (kernel == RT_KERNEL_PIXEL) return rt_launch_pixel(s->spheres_only, s->tex_level, s->need_uv, s->dev, fp, grid, block, stream);
    if (s->spheres_only) {
        if (s->tex_level <= 1) return rt_launch_staged_spheres(s->tex_level, lds_mode, s->dev, fp, grid, block, lds_bytes, stream);
        return rt_launch_staged_spheres_tex(lds_mode, s->dev, fp, grid, block, lds_bytes, stream);
    }
    if (s->tex_level <= 1 && !s->need_uv) return rt_launch_staged_general(lds_mode, s->dev, fp, grid, block, lds_bytes, stream);
    return rt_launch_staged_general_tex(lds_mode, s->dev, fp, grid, block, lds_bytes, stream);
}

}  // namespace

rt_status rt_host::init_device(int device_ordinal) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_last_hip_error = (int)e;
        g_detail = "no HIP device visible (the render path has no CPU fallback)";
        return RT_ERR_NO_DEVICE;
    }
    if (device_ordinal < 0 || device_ordinal >= count || device_ordinal >= RT_MAX_DEVICES) return invalid("device ordinal out of range");
    HIPCHK(hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_ordinal));
    if (!strstr(prop.gcnArchName, "gfx950")) {
        g_detail = std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only";
        return RT_ERR_NO_DEVICE;
    }
    device_info& d = g_devices[device_ordinal];
    d.num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    d.lds_per_cu = prop.maxSharedMemoryPerMultiProcessor > 0 ? (size_t)prop.maxSharedMemoryPerMultiProcessor : (size_t)160 * 1024;
    d.ready = true;
    return RT_OK;
}
rt_status rt_host::rt_internal_init_device(int device_ordinal) {
    const rt_status st = init_device(device_ordinal);
    if (st == RT_OK) g_device = device_ordinal;
    return st;
}

extern "C" {

rt_status rt_init(int device_ordinal) { return rt_internal_init_device(device_ordinal); }

rt_status rt_shutdown(void) {
    for (device_info& d : g_devices) d.ready = false;
    g_device = -1;
    return RT_OK;
}

rt_status rt_reset_options(void) {
    ++g_opt_epoch;
    g_opt = rt_options();
    return RT_OK;
}

const char* rt_strerror(rt_status s) {
    switch (s) {
    case RT_OK: return "ok";
    case RT_ERR_INVALID: return "invalid argument or malformed scene description";
    case RT_ERR_NO_DEVICE: return "no gfx950 HIP device";
    case RT_ERR_HIP: return "HIP runtime error";
    case RT_ERR_UNSUPPORTED: return "unsupported scene construct";
    default: return "unknown status";
    }
}
int rt_last_hip_error(void) { return g_last_hip_error; }
const char* rt_last_error_detail(void) { return g_detail.c_str(); }

rt_status rt_set_option(const char* key, int value) {
    if (!key) return invalid("null option key");
    ++g_opt_epoch;
    const std::string k(key);
    if (k == "kernel") { if (value != RT_KERNEL_PIXEL && value != RT_KERNEL_STAGED) return invalid("kernel: 0 (pixel) or 3 (staged)"); g_opt.kernel = value; }
    else if (k == "leaf_threshold") { if (value < 1 || value > 64) return invalid("leaf_threshold: 1..64"); g_opt.leaf_threshold = value; }
    else if (k == "box_threshold") { if (value < 1 || value > 64) return invalid("box_threshold: 1..64"); g_opt.box_threshold = value; }
    else if (k == "medium_threshold") { if (value < 1 || value > 64) return invalid("medium_threshold: 1..64"); g_opt.medium_threshold = value; }
    else if (k == "diel_threshold") { if (value < 1 || value > 64) return invalid("diel_threshold: 1..64"); g_opt.diel_threshold = value; }
    else if (k == "newpath_threshold") { if (value < 0 || value > 64) return invalid("newpath_threshold: 0 (by kernel family) or 1..64"); g_opt.newpath_threshold = value; }
    else if (k == "sparse_stride") { if (value != 0 && value != 2 && value != 4 && value != 8 && value != 16 && value != 32 && value != 64) return invalid("sparse_stride: 0, 2, 4, ... 64"); g_opt.sparse_stride = value; }
    else if (k == "sparse_factor_x10") { if (value < 10 || value > 1000) return invalid("sparse_factor_x10: 10..1000"); g_opt.sparse_factor_x10 = value; }
    else if (k == "heavy_factor_x10") { if (value < 10 || value > 1000) return invalid("heavy_factor_x10: 10..1000"); g_opt.heavy_factor_x10 = value; }
    else if (k == "tier_auto") { if (value < 0 || value > 1) return invalid("tier_auto: 0 or 1"); g_opt.tier_auto = value; }
    else if (k == "tier_kernel") { if (value < 0 || value > 1) return invalid("tier_kernel: 0 or 1"); g_opt.tier_kernel = value; }
    else if (k == "handoff") { if (value < 0 || value > 1) return invalid("handoff: 0 or 1"); g_opt.handoff = value; }
    else if (k == "handoff_scan") { if (value < 0 || value > 1) return invalid("handoff_scan: 0 or 1"); g_opt.handoff_scan = value; }
    else if (k == "handoff_poll_us") { if (value < 1 || value > 1000000) return invalid("handoff_poll_us: 1..1000000"); g_opt.handoff_poll_us = value; }
    else if (k == "handoff_pixels") { if (value < -1 || value > (1 << 24)) return invalid("handoff_pixels: -1 (auto) or 0..16777216"); g_opt.handoff_pixels = value; }
    else if (k == "handoff_order") { if (value < 0 || value > 1) return invalid("handoff_order: 0 or 1"); g_opt.handoff_order = value; }
    else if (k == "prior") { if (value < 0 || value > 1) return invalid("prior: 0 or 1"); g_opt.prior = value; }
    else if (k == "presplit_samples") { if (value < 0 || value > 4096) return invalid("presplit_samples: 0..4096"); g_opt.presplit_samples = value; }
    else if (k == "resplit_samples") { if (value < 0 || value > 65536) return invalid("resplit_samples: 0..65536"); g_opt.resplit_samples = value; }
    else if (k == "split_samples") { if (value < 1 || value > 4096) return invalid("split_samples: 1..4096"); g_opt.split_samples = value; }
    else if (k == "tier1_factor_x10") { if (value < 10 || value > 10000) return invalid("tier1_factor_x10: 10..10000"); g_opt.tier1_factor_x10 = value; }
    else if (k == "cost_smooth_percent") { if (value < 0 || value > 100) return invalid("cost_smooth_percent: 0..100"); g_opt.cost_smooth_percent = value; }
    else if (k == "tier1_depth") { if (value < 1 || value > 64) return invalid("tier1_depth: 1..64"); g_opt.tier1_depth = value; }
    else if (k == "tier1_pixels") { if (value < 0 || value > 65536) return invalid("tier1_pixels: 0..65536"); g_opt.tier1_pixels = value; }
    else if (k == "semi_stride") { if (value != -1 && value != 0 && value != 1 && value != 2 && value != 4 && value != 8) return invalid("semi_stride: -1 (by kernel family), 0, 1, 2, 4 or 8"); g_opt.semi_stride = value; }
    else if (k == "sparse_eager") { if (value < 0 || value > 1) return invalid("sparse_eager: 0 or 1"); g_opt.sparse_eager = value; }
    else if (k == "tier_priority") { if (value < 0 || value > 3) return invalid("tier_priority: 0..3"); g_opt.tier_priority = value; }
    else if (k == "semi_priority") { if (value < 0 || value > 3) return invalid("semi_priority: 0..3"); g_opt.semi_priority = value; }
    else if (k == "sparse_priority") { if (value < 0 || value > 3) return invalid("sparse_priority: 0..3"); g_opt.sparse_priority = value; }
    else if (k == "sparse_work_percent") { if (value < 0 || value > 100) return invalid("sparse_work_percent: 0..100"); g_opt.sparse_work_percent = value; }
    else if (k == "sparse_wg_percent") { if (value < 1 || value > 100) return invalid("sparse_wg_percent: 1..100"); g_opt.sparse_wg_percent = value; }
    else if (k == "heavy_max_tiles") { if (value < 0 || value > 4096) return invalid("heavy_max_tiles: 0..4096"); g_opt.heavy_max_tiles = value; }
    else if (k == "bvh_collapse") { if (value < 0 || value > 3) return invalid("bvh_collapse: 0..3 (read by rt_scene_create)"); g_opt.bvh_collapse = value; }
    else if (k == "scan_nodes") { if (value < 0 || value > 64) return invalid("scan_nodes: 0..64 (read by rt_scene_create and again by every render's plan)"); g_opt.scan_nodes = value; }
    else if (k == "multi_force_rccl") { if (value < 0 || value > 1) return invalid("multi_force_rccl: 0 or 1"); g_opt.multi_force_rccl = value; }
    else if (k == "cost_map") { if (value < 0 || value > 1) return invalid("cost_map: 0 or 1"); g_opt.cost_map = value; }
    else if (k == "lpt") { if (value < 0 || value > 1) return invalid("lpt: 0 or 1"); g_opt.lpt = value; }
    else if (k == "threads") { if (value != 0 && (value < 64 || value > 768 || (value % 64))) return invalid("threads: 0 (per kernel family) or a multiple of 64 up to 768 (512 for the lean spheres-only kernels)"); g_opt.threads = value; }
    else if (k == "lds_mode") { if (value < -1 || value > 4) return invalid("lds_mode: -1..4"); g_opt.lds_mode = value; }
    else if (k == "steps_per_trip") { if (value < 1 || value > 64) return invalid("steps_per_trip: 1..64"); g_opt.steps_per_trip = value; }
    else if (k == "shade_threshold") { if (value < 0 || value > 64) return invalid("shade_threshold: 0 (by the launch's load) or 1..64"); g_opt.shade_threshold = value; }
    else if (k == "trace_lds") { if (value < -1 || value > 2) return invalid("trace_lds: -1 (auto) .. 2"); g_opt.trace_lds = value; }
    else if (k == "radiance_lds") { if (value < -1 || value > 2) return invalid("radiance_lds: -1 (auto) .. 2"); g_opt.radiance_lds = value; }
    else if (k == "aov_lds") { if (value < -1 || value > 2) return invalid("aov_lds: -1 (auto) .. 2"); g_opt.aov_lds = value; }
    else if (k == "aov_through_lds") { if (value < -1 || value > 2) return invalid("aov_through_lds: -1 (auto) .. 2"); g_opt.aov_through_lds = value; }
    else if (k == "denoise_lds") { if (value < -1 || value > 1) return invalid("denoise_lds: -1 (auto), 0 (direct) or 1 (staged)"); g_opt.denoise_lds = value; }
    else if (k == "upscale_lds") { if (value < -1 || value > 1) return invalid("upscale_lds: -1 (auto), 0 (direct) or 1 (staged)"); g_opt.upscale_lds = value; }
    else if (k == "trace_tree") { if (value < 0 || value > 1) return invalid("trace_tree: 0 (reference tree) or 1 (walk array)"); g_opt.trace_tree = value; }
    else if (k == "adaptive_tier") { if (value < -1 || value > 1) return invalid("adaptive_tier: -1 (auto), 0 (main kernel) or 1 (tier kernel)"); g_opt.adaptive_tier = value; }
    else if (k == "wg_per_cu") { if (value < 0 || value > 8) return invalid("wg_per_cu: 0 (per kernel family) .. 8"); g_opt.wg_per_cu = value; }
    else return invalid("unknown option");
    return RT_OK;
}

rt_status rt_scene_destroy(rt_scene* s) {
    if (!s) return RT_OK;
    (void)use_device(s->device);
    for (hipEvent_t e : s->adapt_events) (void)hipEventDestroy(e);
    if (s->tier_stream) (void)hipStreamDestroy(s->tier_stream);
    for (int k = 0; k < 4; ++k) { if (s->ev_fork[k]) (void)hipEventDestroy(s->ev_fork[k]); if (s->ev_join[k]) (void)hipEventDestroy(s->ev_join[k]); }
    if (s->ev_start) (void)hipEventDestroy(s->ev_start);
    if (s->ev_stop) (void)hipEventDestroy(s->ev_stop);
    delete s;   // (its buffers free themselves: the device is current)
    return RT_OK;
}

namespace {
// the rows of an upload table in their order, each a scene's allocation from then on (rt_scene_destroy frees it)
rt_status upload_arrays(rt_scene* s, std::initializer_list<array_upload> table) {
    for (const array_upload& u : table) {
        *u.dst = nullptr;
        owned<char> copy;
        RT_TRY(upload(u.src, u.bytes, copy));
        *u.dst = copy.get();
        s->allocs.push_back(std::move(copy));
    }
    return RT_OK;
}

// The calibration pass: a small frame through the scene's own camera by kernel 0 with its counters on, which walks `d_tree`
// (n_tree nodes in the device's encoding) in the place of the reference's tree.
struct calibration_request {
    const rt_node* d_tree;
    int n_tree;
    uint32_t sample_stride;   // > 0: every sample_stride-th ray of the pass is kept (the caller knows how many there will be and keeps that
                              // below the capacity, so the SET of sampled rays does not depend on the order the lanes get there)
    bool keep_cost;           // the pass's per-pixel ray counts stay in the scene as the cost prior of ranked first parts (rt_prior_kernel)
};
struct calibration_result {
    std::vector<double> pass;    // per node: the box tests it passed
    double rays = 0.0;
    std::vector<float> sample;   // seven floats per kept ray: origin, direction, the limit it ended with
};
rt_status measure_pass_counts(rt_scene* s, const calibration_request& rq, calibration_result& out) {
    const rt_camera& c = s->dev.camera;
    const double hw = sqrt((double)c.horizontal[0] * c.horizontal[0] + (double)c.horizontal[1] * c.horizontal[1] + (double)c.horizontal[2] * c.horizontal[2]);
    const double vh = sqrt((double)c.vertical[0] * c.vertical[0] + (double)c.vertical[1] * c.vertical[1] + (double)c.vertical[2] * c.vertical[2]);
    double aspect = (hw > 0 && vh > 0) ? hw / vh : 1.0;
    if (!(aspect > 0.05 && aspect < 20.0)) aspect = 1.0;
    int nx = aspect >= 1.0 ? 256 : (int)(256 * aspect + 0.5), ny = aspect >= 1.0 ? (int)(256 / aspect + 0.5) : 256;
    if (nx < 8) nx = 8;
    if (ny < 8) ny = 8;
    const size_t n = (size_t)rq.n_tree;
    rt_scene_dev dev = s->dev;
    dev.nodes_ref = rq.d_tree; dev.n_nodes_ref = rq.n_tree;
    enum { SAMPLE_CAP = 8192 };
    owned<unsigned int> cost;  // (before mem: freed after mem's wait)
    call_memory mem;          // the pass runs on the null stream and is waited for below
    mem.guard(nullptr);
    unsigned int* d_pass = nullptr;
    float *d_fb = nullptr, *d_sample = nullptr;
    HIPCHK(mem.get((void**)&d_pass, n * sizeof(unsigned int)));
    HIPCHK(mem.get((void**)&d_fb, (size_t)nx * ny * 3 * sizeof(float)));
    if (rq.keep_cost) (void)cost.grow((size_t)nx * ny);   // (a failure: no prior then)
    if (rq.sample_stride > 0 && mem.get((void**)&d_sample, (size_t)SAMPLE_CAP * 7 * sizeof(float)) != hipSuccess) d_sample = nullptr;   // no sample then
    rt_frame_params fp;
    memset(&fp, 0, sizeof(fp));
    fp.fb = d_fb; fp.ray_counter = s->d_ray_counter; fp.work_counter = s->d_work_counter; fp.node_pass = d_pass; fp.pixel_cost = cost;
    fp.node_pass_lds = n * sizeof(unsigned int) <= 48u * 1024u ? 1 : 0;
    fp.seed_base = 1984; fp.nx = nx; fp.ny = ny; fp.ns = 4; fp.gamma = 1.0f;
    fp.tile_rows = ny; fp.tile_first = 0; fp.tile_stride = 1; fp.local_rows = ny;
    fp.tiles_x = tiles_across(nx);
    fp.work_items = (uint32_t)fp.tiles_x * (uint32_t)tiles_across(ny) * 64u;
    fp.sample_begin = 0; fp.sample_end = fp.ns;
    if (d_sample) { fp.ray_sample = d_sample; fp.ray_sample_cap = SAMPLE_CAP; fp.ray_sample_stride = rq.sample_stride; }
    std::vector<unsigned int> h(n);
    unsigned long long r = 0;
    const hipError_t e = [&]() -> hipError_t {
        hipError_t e;
        if ((e = hipMemset(d_pass, 0, n * sizeof(unsigned int))) != hipSuccess) return e;
        if ((e = hipMemset(s->d_ray_counter, 0, RT_COUNTER_BYTES)) != hipSuccess) return e;
        if ((e = rt_launch_pixel(s->spheres_only, s->tex_level, s->need_uv, dev, fp, dim3((fp.work_items + 255u) / 256u), dim3(256), nullptr)) != hipSuccess) return e;
        if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
        if ((e = hipMemcpy(h.data(), d_pass, n * sizeof(unsigned int), hipMemcpyDeviceToHost)) != hipSuccess) return e;
        if ((e = hipMemcpy(&r, s->d_ray_counter, sizeof(r), hipMemcpyDeviceToHost)) != hipSuccess) return e;
        if (d_sample) {
            unsigned long long taken = 0;
            if ((e = hipMemcpy(&taken, s->d_ray_counter + 2, sizeof(taken), hipMemcpyDeviceToHost)) != hipSuccess) return e;
            if (taken > SAMPLE_CAP) taken = SAMPLE_CAP;
            out.sample.resize((size_t)taken * 7);
            if (taken && (e = hipMemcpy(out.sample.data(), d_sample, (size_t)taken * 7 * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) return e;
        }
        return hipSuccess;
    }();
    if (e != hipSuccess) { g_last_hip_error = (int)e; g_detail = std::string("calibration pass: ") + hipGetErrorString(e); return RT_ERR_HIP; }
    mem.settled();
    if (cost) {   // the scene's prior from now on, in the place of the one it had
        s->d_cal_cost.adopt(cost.release(), (size_t)nx * ny);
        s->cal_nx = nx; s->cal_ny = ny;
    }
    out.pass.assign(h.begin(), h.end());
    out.rays = (double)r;
    return RT_OK;
}
// the cost half of the calibration alone, for a scene that kept a prior at creation (one that kept none gets none: a fresh scene
// would have none either): the pass on the reference's tree with keep_cost, its pass counts dropped
rt_status recalibrate_cost(rt_scene* s) {
    if (!s->d_cal_cost) return RT_OK;
    calibration_result dropped;
    return measure_pass_counts(s, {s->dev.nodes_ref, s->dev.n_nodes_ref, 0, true}, dropped);
}

// uploads the tier data (rt_scene_plan.h) and points dev at them; a scene that gets none keeps the null arrays
rt_status build_tier_data(rt_scene* s, const rt_scene_desc* d) {
    const rt_scene_plan::tier_data t = rt_scene_plan::plan_tier_data(d);
    const float *d_lo = nullptr, *d_hi = nullptr, *d_ranges = nullptr;
    if (t.present) RT_TRY(upload_arrays(s, {array_of(t.lo, &d_lo), array_of(t.hi, &d_hi), array_of(t.ranges, &d_ranges)}));
    s->dev.leaf_lo = reinterpret_cast<const float4*>(d_lo); s->dev.leaf_hi = reinterpret_cast<const float4*>(d_hi); s->dev.slot_ranges = d_ranges;
    s->dev.n_leaves = t.n_leaves; s->dev.n_slots = t.n_slots; s->dev.n_media_leaves = t.n_media_leaves;
    s->dev.media_ord[0] = t.media_ord[0]; s->dev.media_ord[1] = t.media_ord[1];
    return RT_OK;
}

// builds the walk array ("Collapse" and "Regroup", rt_scene_plan.h) and points dev.nodes at it
rt_status build_walk(rt_scene* s, const rt_scene_desc* d) {
    using namespace rt_scene_plan;
    const int n = d->n_nodes;
    s->walk_tests_before = s->walk_tests_after = 0.0;
    if (g_opt.bvh_collapse == 0 || n < 3) return RT_OK;
    calibration_result ref;   // of the reference's tree
    if (g_opt.bvh_collapse >= 2) RT_TRY(measure_pass_counts(s, {s->dev.nodes_ref, n, 0, true}, ref));
    const bool measured = ref.rays > 0.0;
    if (!measured) { ref.pass = area_passes(d->nodes, n); ref.rays = ref.pass[0]; }
    const double root_visits = ref.rays;
    collapse_plan plan;
    const bool planned = plan_collapse(d->nodes, n, ref.pass, root_visits, plan);
    std::vector<rt_node> walk;
    if (planned) walk = build_walk_array(d->nodes, n, plan.keep);
    bool changed = planned && (int)walk.size() != n;
    // the regrouped hierarchies over the same leaves, through the same calibration pass and DP; they need the reference's own
    // tree to have passed the checks (a real tree, boxes containing their children's)
    if (g_opt.bvh_collapse >= 3 && measured && planned) {
        // bounds on the planning time of very large scenes (the reference's have at most 1410 leaves): the top-down split is
        // quadratic in the worst case, the sampled-ray key costs leaves x rays
        int n_leaves = 0;
        for (int i = 0; i < n; ++i) n_leaves += d->nodes[i].prim >= 0 ? 1 : 0;
        std::vector<float> ray_sample;
        for (int method = 0; method < 3; ++method) {
            if (method == 0 && n_leaves > 65536) continue;
            if (method == 2 && (ray_sample.size() < 7 * 256 || n_leaves > 8192)) continue;
            const std::vector<rt_node> tree = regroup_leaves(d->nodes, n, method, &ray_sample);
            const int m = (int)tree.size();
            if (m < 3) continue;
            owned<char> d_tree;   // the candidate on the device
            RT_TRY(upload(device_nodes(tree.data(), tree.size()).data(), tree.size() * sizeof(rt_node), d_tree));
            // the first of these passes also keeps ~4000 of its rays for method 2 (same frame, same rays in every pass)
            calibration_result c;
            RT_TRY(measure_pass_counts(s, {reinterpret_cast<const rt_node*>(d_tree.get()), m, method == 0 ? (uint32_t)(root_visits / 4096.0) + 1u : 0u, false}, c));
            if (method == 0) ray_sample.swap(c.sample);
            collapse_plan plan2;
            const bool ok2 = c.rays == root_visits && plan_collapse(tree.data(), m, c.pass, c.rays, plan2);
            if (ok2 && plan2.tests_after < plan.tests_after) {
                walk = build_walk_array(tree.data(), m, plan2.keep);
                plan.tests_after = plan2.tests_after;            // "before" stays the reference tree's figure
                changed = true;
            }
        }
    }
    {   // (the estimates stay the plan's: per-lane box tests of the array a walk would use)
        std::vector<rt_node> cur = changed ? walk : std::vector<rt_node>(d->nodes, d->nodes + n);
        if (leaves_only_if_scanned(cur.data(), (int)cur.size(), g_opt.scan_nodes, walk)) changed = true;
    }
    if (!changed) return RT_OK;
    RT_TRY(upload_arrays(s, {array_of(device_nodes(walk.data(), walk.size()), &s->dev.nodes)}));
    s->dev.n_nodes = (int32_t)walk.size();
    s->walk_tests_before = plan.tests_before; s->walk_tests_after = plan.tests_after;
    return RT_OK;
}

// the per-frame resources of a new scene: the counters, the frame's events, and the tier kernel's stream with the events that
// fork it from / join it to the caller's stream, one pair per ranked part
rt_status create_frame_resources(rt_scene* s) {
    hipError_t e;
    if ((e = (hipError_t)s->d_ray_counter.grow(RT_COUNTER_BYTES / 8)) != hipSuccess || (e = (hipError_t)s->d_work_counter.grow(RT_WORK_COUNTER_BYTES / 4)) != hipSuccess ||
        (e = hipEventCreate(&s->ev_start)) != hipSuccess || (e = hipEventCreate(&s->ev_stop)) != hipSuccess) {
        g_last_hip_error = (int)e; g_detail = "allocating per-frame resources failed";
        return RT_ERR_HIP;
    }
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    e = hipStreamCreateWithPriority(&s->tier_stream, hipStreamNonBlocking, prio_hi);
    for (int k = 0; k < 4 && e == hipSuccess; ++k) {
        e = hipEventCreateWithFlags(&s->ev_fork[k], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_join[k], hipEventDisableTiming);
    }
    if (e != hipSuccess) { g_last_hip_error = (int)e; g_detail = "creating the tier stream failed"; return RT_ERR_HIP; }
    return RT_OK;
}
}  // namespace

rt_status rt_scene_create(const rt_scene_desc* d, rt_scene** out) {
    if (!out) return invalid("null output pointer");
    *out = nullptr;
    if (g_device < 0) { g_detail = "rt_init has not succeeded"; return RT_ERR_NO_DEVICE; }
    return rt_internal_scene_create_on(g_device, d, out);
}

}  // extern "C"

// (shared with rt_multi.hip: rt_host.h)
rt_status rt_host::rt_internal_scene_create_on(int device, const rt_scene_desc* d, rt_scene** out) {
    if (!out) return invalid("null output pointer");
    *out = nullptr;
    RT_TRY(use_device(device));
    rt_scene_plan::scene_class cls;
    if (const char* why = rt_scene_plan::validate(d, cls)) return invalid(why);
    // what the device gets in place of the description's arrays: the nodes in its link encoding, quads, boxes and materials marked
    const std::vector<rt_node> nodes = rt_scene_plan::device_nodes(d->nodes, (size_t)d->n_nodes);
    const std::vector<rt_quad> quads = rt_scene_plan::marked_quads(d);
    const std::vector<rt_box> boxes = rt_scene_plan::marked_boxes(d);
    const std::vector<rt_material> materials = rt_scene_plan::marked_materials(d);

    rt_scene* s = new rt_scene;
    s->device = device;
    memset(&s->dev, 0, sizeof(s->dev));
    memset(&s->pending_stats, 0, sizeof(s->pending_stats));
    s->spheres_only = cls.spheres_only; s->tex_level = cls.tex_level; s->need_uv = cls.need_uv;
    rt_scene_dev& dev = s->dev;
    rt_status st = upload_arrays(s, {
        array_of(nodes, &dev.nodes_ref), array_of(d->spheres, (size_t)d->n_spheres, &dev.spheres), array_of(quads, &dev.quads), array_of(boxes, &dev.boxes),
        array_of(d->instances, (size_t)d->n_instances, &dev.instances), array_of(d->media, (size_t)d->n_media, &dev.media), array_of(materials, &dev.materials),
        array_of(d->textures, (size_t)d->n_textures, &dev.textures), array_of(d->images, d->image_bytes, &dev.images)});
    dev.nodes = dev.nodes_ref; dev.n_nodes = dev.n_nodes_ref = d->n_nodes;     // until the walk array is built below
    dev.n_spheres = d->n_spheres; dev.n_materials = d->n_materials; dev.n_textures = d->n_textures;
    rt_scene_plan::axis_bound(d->nodes, d->n_nodes, dev.bound);
    dev.bound_pad = 0.0f;
    dev.camera = d->camera;
    s->n_instances = d->n_instances; s->n_media = d->n_media;
    s->n_quads = d->n_quads; s->n_boxes = d->n_boxes;
    s->refit.instanced = rt_refit::instanced_spheres(d->instances, d->n_instances, d->n_spheres);   // (host only: an update's checks need no HIP call)
    for (int i = 0; i < d->n_instances; ++i) s->refit.inst_child.push_back(d->instances[i].child);
    s->shade_bytes = (size_t)d->n_materials * sizeof(rt_material) + (size_t)d->n_textures * sizeof(rt_texture);
    s->sphere_bytes = (size_t)d->n_spheres * sizeof(rt_sphere);
    if (st == RT_OK) st = create_frame_resources(s);
    if (st == RT_OK) st = build_tier_data(s, d);
    if (st == RT_OK) st = build_walk(s, d);
    if (st != RT_OK) { rt_scene_destroy(s); return st; }
    s->node_bytes = (size_t)dev.n_nodes * sizeof(rt_node);
    *out = s;
    return RT_OK;
}

extern "C" {

// Host-only: the walk array rt_scene_create would build for `nodes` given per-node pass counts (`pass`, one per node;
// null = proportional to box surface area) and `root_visits` rays.  Writes at most `cap` nodes to `out`, returns the
// walk array's size through `n_out` and the expected box tests per ray before / after.  No device involved.
rt_status rt_plan_walk_array(const rt_node* nodes, int32_t n, const double* pass, double root_visits, rt_node* out, int32_t cap,
                             int32_t* n_out, double* tests_before, double* tests_after) {
    if (!nodes || n <= 0 || !n_out) return invalid("rt_plan_walk_array: bad argument");
    for (int i = 0; i < n; ++i) if (nodes[i].skip <= i || nodes[i].skip > n) return invalid("node skip link does not move forward");
    const std::vector<double> p = pass ? std::vector<double>(pass, pass + n) : rt_scene_plan::area_passes(nodes, n);
    if (!pass) root_visits = p[0];
    rt_scene_plan::collapse_plan plan;
    std::vector<rt_node> walk(nodes, nodes + n);
    if (rt_scene_plan::plan_collapse(nodes, n, p, root_visits, plan)) walk = rt_scene_plan::build_walk_array(nodes, n, plan.keep);
    *n_out = (int32_t)walk.size();
    if (tests_before) *tests_before = plan.tests_before;
    if (tests_after) *tests_after = plan.tests_after;
    if (out) for (int i = 0; i < (int)walk.size() && i < cap; ++i) out[i] = walk[i];
    return RT_OK;
}

rt_status rt_regroup_leaves(const rt_node* nodes, int32_t n, int32_t method, rt_node* out, int32_t cap, int32_t* n_out) {
    if (!nodes || n <= 0 || !n_out || method < 0 || method > 1) return invalid("rt_regroup_leaves: bad argument");
    const std::vector<rt_node> tree = rt_scene_plan::regroup_leaves(nodes, n, method);
    *n_out = (int32_t)tree.size();
    if (out) for (int i = 0; i < (int)tree.size() && i < cap; ++i) out[i] = tree[i];
    return RT_OK;
}

rt_status rt_scene_walk_info(const rt_scene* s, int32_t* nodes_reference, int32_t* nodes_walked, double* tests_before, double* tests_after) {
    if (!s) return invalid("null scene");
    if (nodes_reference) *nodes_reference = s->dev.n_nodes_ref;
    if (nodes_walked) *nodes_walked = s->dev.n_nodes;
    if (tests_before) *tests_before = s->walk_tests_before;
    if (tests_after) *tests_after = s->walk_tests_after;
    return RT_OK;
}

namespace {
// where the kernels write the frame: the caller's device buffer, or the scene's image of a host buffer (`floats` floats)
rt_status device_fb(rt_scene* s, float* fb, int fb_on_device, size_t floats, float** d_fb) {
    if (!fb_on_device) HIPCHK(s->d_fb.grow(floats));
    *d_fb = fb_on_device ? fb : s->d_fb;
    return RT_OK;
}

}  // namespace

int32_t rt_frame_local_rows(const rt_frame_desc* f) {
    if (!f || f->ny <= 0 || f->tile_rows <= 0 || f->tile_stride <= 0 || f->tile_first < 0) return -1;
    const int n_tiles = (f->ny + f->tile_rows - 1) / f->tile_rows;
    int rows = 0;
    for (int t = f->tile_first; t < n_tiles; t += f->tile_stride) {
        const int r0 = t * f->tile_rows;
        const int r1 = r0 + f->tile_rows < f->ny ? r0 + f->tile_rows : f->ny;
        rows += r1 - r0;
    }
    return rows;
}

int32_t rt_local_to_global_row(const rt_frame_desc* f, int32_t local_row) {
    if (!f || f->tile_rows <= 0) return -1;
    const int t = local_row / f->tile_rows;
    return (f->tile_first + t * f->tile_stride) * f->tile_rows + (local_row - t * f->tile_rows);
}

rt_status rt_frame_finish(rt_scene* s, rt_stats* stats) {
    if (!s) return invalid("null scene");
    if (!s->frame_pending) { if (stats) *stats = s->pending_stats; return RT_OK; }
    RT_TRY(use_device(s->device));
    HIPCHK(hipEventSynchronize(s->ev_stop));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, s->ev_start, s->ev_stop));
    unsigned long long rays = 0;
    HIPCHK(hipMemcpy(&rays, s->d_ray_counter, sizeof(rays), hipMemcpyDeviceToHost));
    s->pending_stats.ms_render = (double)ms;
    s->pending_stats.rays = rays;
    if (s->plan.ranked && s->d_rank) {   // how many pixels the last ranking listed as heavy (diagnostics)
        rt_rank_info inf;
        HIPCHK(hipMemcpy(&inf, s->d_rank, sizeof(inf), hipMemcpyDeviceToHost));
        s->pending_stats.reserved = (int32_t)inf.heavy_items;
    }
    s->frame_pending = false;
    if (s->cost_map.pending) {   // the frame that wrote the cost map is complete
        s->cost_map.pending = false; s->cost_map.valid = rays > 0; s->cost_map.total = rays;
    }
    if (stats) *stats = s->pending_stats;
    return RT_OK;
}

namespace {
// the checks rt_scene_set_camera and rt_reproject make of a camera: every field finite (pad is not looked at), time0 <= time1
const char* camera_fault(const rt_camera& c) {
    const float* groups[6] = {c.origin, c.lower_left_corner, c.horizontal, c.vertical, c.u, c.v};
    for (const float* g : groups)
        for (int k = 0; k < 3; ++k) if (!std::isfinite(g[k])) return "a camera field is not finite";
    if (!std::isfinite(c.lens_radius) || !std::isfinite(c.time0) || !std::isfinite(c.time1)) return "a camera field is not finite";
    if (c.time1 < c.time0) return "the camera's time1 is before its time0";
    return nullptr;
}
}  // namespace

// ---- rt_scene_set_camera (include/rt_abi.h).  The camera lives in rt_scene_dev, which every launch copies into
// its kernel's argument block: replacing it is the whole change.  The walk array, the tier data and the LDS plans do not depend
// on it.  recalibrate: the cost half of the calibration alone -- the pass of build_walk on the reference's tree with keep_cost,
// its pass counts dropped.
rt_status rt_scene_set_camera(rt_scene* s, const rt_camera* camera, int recalibrate) {
    if (!s) return invalid("rt_scene_set_camera: null scene");
    if (!camera) return invalid("rt_scene_set_camera: null camera");
    if (const char* why = camera_fault(*camera)) return invalid((std::string("rt_scene_set_camera: ") + why).c_str());
    RT_TRY(use_device(s->device));
    if (s->frame_pending) RT_TRY(rt_frame_finish(s, nullptr));
    s->dev.camera = *camera;
    ++s->scene_epoch;                                // the cost map is stale ...
    if (recalibrate) s->cost_map.valid = false;      // ... or, with a fresh calibration prior asked for, dropped
    if (recalibrate) RT_TRY(recalibrate_cost(s));
    return RT_OK;
}

rt_status rt_scene_get_camera(const rt_scene* s, rt_camera* out) {
    if (!s) return invalid("rt_scene_get_camera: null scene");
    if (!out) return invalid("rt_scene_get_camera: null output pointer");
    *out = s->dev.camera;
    return RT_OK;
}

namespace {
// a pointer rt_trace_rays / rt_radiance_rays (`who`) hands to a kernel: null, or `bytes` of device (or managed) memory of
// `device`, aligned to `align` bytes
rt_status check_trace_ptr(const void* p, size_t bytes, int device, const char* what, const char* who, unsigned align) {
    if (!p) return RT_OK;
    std::string why;
    if (reinterpret_cast<uintptr_t>(p) & (align - 1u)) { why = std::string(who) + ": " + what + " is not " + std::to_string(align) + "-byte aligned"; return invalid(why.c_str()); }
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        why = std::string(who) + ": " + what + " is not device memory (unregistered pointer)";
        return invalid(why.c_str());
    }
    if (a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged) {
        why = std::string(who) + ": " + what + " is not device memory";
        return invalid(why.c_str());
    }
    if (a.type == hipMemoryTypeDevice && a.device != device) {
        why = std::string(who) + ": " + what + " is memory of another device";
        return invalid(why.c_str());
    }
    void* base = nullptr;
    size_t size = 0;
    if (a.type == hipMemoryTypeDevice && hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) == hipSuccess) {
        if (static_cast<const char*>(p) + bytes > static_cast<const char*>(base) + size) {
            why = std::string(who) + ": " + what + " is shorter than the batch";
            return invalid(why.c_str());
        }
    } else {
        (void)hipGetLastError();
    }
    return RT_OK;
}
// a table of such pointers (traced_ptr, rt_call_buffers.h), checked in its order
extern "C++" template <class Table> rt_status check_trace_ptrs(const Table& table, int device, const char* who) {
    for (const traced_ptr& q : table) RT_TRY(check_trace_ptr(q.p, q.bytes, device, q.what, who, q.align));
    return RT_OK;
}

// The image-space entries (rt_render_aov*, rt_denoise*, rt_upscale, rt_reproject*) keep their buffers in a table of call_buffer
// (rt_call_buffers.h) beside dev[], the pointers their kernels get.  For host buffers those are images in one allocation of the
// call's own, behind `lead` bytes the entry keeps for itself (`base`, if it asks for them): of the buffers for which used(k), in
// table order.  (A HIP error in these helpers is reported with the helper's line and expression, not the entry's.)
extern "C++" template <class Table, class Used>
rt_status stage_buffers(call_memory& mem, const Table& table, Used used, const void** dev, size_t lead = 0, char** base = nullptr) {
    char* memory = nullptr;
    HIPCHK(mem.get((void**)&memory, staged_bytes(table, used, lead)));
    place_staged(table, used, memory, lead, dev);
    if (base) *base = memory;
    return RT_OK;
}
// ... the used inputs go up and the given outputs come down on the call's stream
extern "C++" template <class Table, class Used> rt_status upload_inputs(const Table& table, Used used, const void* const* dev, hipStream_t stream) {
    int k = 0;
    for (const call_buffer& b : table) {
        if (used(k) && b.role == BUF_INPUT) HIPCHK(hipMemcpyAsync(const_cast<void*>(dev[k]), b.p, b.bytes, hipMemcpyHostToDevice, stream));
        ++k;
    }
    return RT_OK;
}
extern "C++" template <class Table> rt_status download_outputs(const Table& table, const void* const* dev, hipStream_t stream) {
    int k = 0;
    for (const call_buffer& b : table) {
        if (b.p && b.role == BUF_OUTPUT) HIPCHK(hipMemcpyAsync(const_cast<void*>(b.p), dev[k], b.bytes, hipMemcpyDeviceToHost, stream));
        ++k;
    }
    return RT_OK;
}

// LDS residency and the persistent grid of the one-item-per-lane kernels (rt_trace_rays, rt_radiance_rays, rt_render_aov) for a
// node array of `node_bytes`: the modes whose image fits a CU (2 = nodes + spheres, 1 = nodes only, 0 = none); a forced mode
// (`option` >= 0) that does not fit falls back to the largest that does.  Auto (`option` < 0) takes the largest mode that keeps
// at least 3/4 of the workgroups per CU that mode 0 gets: the walk is latency-bound, and an image that costs residency costs
// more than it saves -- one workgroup per CU for the Book-2 final scene's nodes ran at 0.6 instead of 1.4 Grays/s; the headline
// scene's nodes (7 of 8 workgroups) were 1-8 % faster than mode 0 (profiles/trace_bench_mi355x.jsonl).
// occupancy(mode, lds bytes, &workgroups per CU) asks the kernel that would be launched.  The grid holds as many workgroups
// as are resident at once (registers and LDS), never more than `need`.
struct resident_plan { int lds_mode; size_t lds; dim3 grid; };
rt_status plan_resident(const rt_scene* s, size_t node_bytes, int option, long long need,
                        const std::function<hipError_t(int, size_t, int*)>& occupancy, resident_plan& plan) {
    const size_t budget = g_devices[s->device].lds_per_cu - 2048;
    const int fit = node_bytes + s->sphere_bytes <= budget ? 2 : (node_bytes <= budget ? 1 : 0);
    auto lds_of = [&](int m) -> size_t { return m == 2 ? node_bytes + s->sphere_bytes : (m == 1 ? node_bytes : 0); };
    int lds_mode = option < 0 ? fit : std::min(option, fit);
    int per_cu = 0;
    HIPCHK(occupancy(lds_mode, lds_of(lds_mode), &per_cu));
    if (option < 0 && lds_mode > 0) {
        int per_cu0 = 0;
        HIPCHK(occupancy(0, (size_t)0, &per_cu0));
        while (lds_mode > 0 && 4 * per_cu < 3 * per_cu0) {
            --lds_mode;
            HIPCHK(occupancy(lds_mode, lds_of(lds_mode), &per_cu));
        }
    }
    if (per_cu < 1) per_cu = 1;
    const long long want = (long long)g_devices[s->device].num_cu * per_cu;
    plan.lds_mode = lds_mode;
    plan.lds = lds_of(lds_mode);
    plan.grid = dim3((unsigned)std::min(want, need));
    return RT_OK;
}
}  // namespace

// ---- rt_scene_update_spheres, rt_scene_update_instances, rt_scene_update_quads (include/rt_abi.h).
// Nothing of the scene's topology changes: the kernels of rt_kernel_refit.hip store the records and recompute, where they live, the
// boxes that depend on them.  The three kinds share the tables, the launches and the body below (update_records).
namespace {
// The lookup tables, once per scene: the node arrays are read back (the device holds the only copy of the walk array) and every
// node's subtree -- nodes [i, skip[i]) of a depth-first array -- becomes a range of leaf ordinals.
rt_status build_refit_tables(rt_scene* s) {
    rt_scene::refit_tables& t = s->refit;
    if (t.ready) return RT_OK;
    const bool own_walk = s->dev.nodes != s->dev.nodes_ref;
    const int n_ref = s->dev.n_nodes_ref, n_walk = own_walk ? s->dev.n_nodes : 0;
    std::vector<rt_node> ref((size_t)n_ref), walk((size_t)n_walk);
    std::vector<rt_medium> media((size_t)s->n_media);
    if (n_ref) HIPCHK(hipMemcpy(ref.data(), s->dev.nodes_ref, ref.size() * sizeof(rt_node), hipMemcpyDeviceToHost));
    if (n_walk) HIPCHK(hipMemcpy(walk.data(), s->dev.nodes, walk.size() * sizeof(rt_node), hipMemcpyDeviceToHost));
    if (s->n_media) HIPCHK(hipMemcpy(media.data(), s->dev.media, media.size() * sizeof(rt_medium), hipMemcpyDeviceToHost));

    // leaves by ordinal, and one job per interior node: (node, first leaf, end leaf, array)
    std::vector<int32_t> leaf_solid, leaf_node_ref, leaf_node_walk;
    std::vector<float> box_lo, box_hi;
    std::vector<int4> jobs;
    auto scan = [&](const std::vector<rt_node>& nodes, int which, std::vector<int32_t>& leaf_node) -> bool {
        const int n = (int)nodes.size();
        std::vector<int32_t> before((size_t)n + 1, 0);             // leaves among nodes [0, i)
        for (int i = 0; i < n; ++i) before[(size_t)i + 1] = before[(size_t)i] + (nodes[i].prim >= 0 ? 1 : 0);
        for (int i = 0; i < n; ++i) {
            const int skip = RT_NODE_SKIP(nodes[i].skip);
            if (skip <= i || skip > n) return false;
            if (nodes[i].prim >= 0) leaf_node.push_back(i);
            else jobs.push_back(make_int4(i, before[(size_t)i], before[(size_t)skip], which));
        }
        return true;
    };
    if (!scan(ref, 0, leaf_node_ref) || !scan(walk, 1, leaf_node_walk)) return invalid("rt_scene_update_spheres: the scene's node links are damaged");
    const int m = (int)leaf_node_ref.size();
    if (own_walk && (int)leaf_node_walk.size() != m) return invalid("rt_scene_update_spheres: the walk array does not hold the reference tree's leaves");
    if (s->dev.leaf_lo && s->dev.n_leaves != m) return invalid("rt_scene_update_spheres: the tier data do not hold the reference tree's leaves");
    const int slots = (m + 63) / 64;
    leaf_solid.assign((size_t)m, -1);
    box_lo.assign((size_t)slots * 64 * 4, 0.0f); box_hi.assign((size_t)slots * 64 * 4, 0.0f);
    for (int q = 0; q < m; ++q) {
        const rt_node& n = ref[(size_t)leaf_node_ref[(size_t)q]];
        if (own_walk && walk[(size_t)leaf_node_walk[(size_t)q]].prim != n.prim) return invalid("rt_scene_update_spheres: the walk array's leaves are not in the reference tree's order");
        leaf_solid[(size_t)q] = rt_refit::leaf_solid(n.prim, media.data(), s->n_media, s->dev.n_spheres, s->n_quads, s->n_boxes, s->n_instances);
        for (int c = 0; c < 3; ++c) { box_lo[(size_t)q * 4 + c] = n.bmin[c]; box_hi[(size_t)q * 4 + c] = n.bmax[c]; }
    }
    if (!own_walk) leaf_node_walk.clear();

    // one block, every piece 256-byte aligned: the three stamp arrays, the three leaf tables, the canonical boxes, slot unions and maxima, jobs, result
    const bool tier = s->dev.slot_ranges != nullptr;
    struct piece { size_t bytes; const void* src; void** dst; };
    int32_t *d_lq = nullptr, *d_lr = nullptr, *d_lw = nullptr; float4 *d_lo = nullptr, *d_hi = nullptr;
    float *d_slot = nullptr, *d_abs = nullptr, *d_result = nullptr; int4* d_jobs = nullptr;
    const piece pieces[] = {
        {(size_t)s->dev.n_spheres * 4, nullptr, (void**)&t.stamp[rt_refit::SPHERES]},
        {(size_t)s->n_instances * 4, nullptr, (void**)&t.stamp[rt_refit::INSTANCES]},
        {(size_t)s->n_quads * 4, nullptr, (void**)&t.stamp[rt_refit::QUADS]},
        {leaf_solid.size() * 4, leaf_solid.data(), (void**)&d_lq},
        {leaf_node_ref.size() * 4, leaf_node_ref.data(), (void**)&d_lr},
        {leaf_node_walk.size() * 4, leaf_node_walk.data(), (void**)&d_lw},
        {box_lo.size() * 4, box_lo.data(), (void**)&d_lo},
        {box_hi.size() * 4, box_hi.data(), (void**)&d_hi},
        {tier ? 0 : (size_t)slots * 32, nullptr, (void**)&d_slot},
        {(size_t)slots * 16, nullptr, (void**)&d_abs},
        {jobs.size() * sizeof(int4), jobs.data(), (void**)&d_jobs},
        {16, nullptr, (void**)&d_result},
    };
    size_t total = 0;
    for (const piece& pc : pieces) total += call_memory::rounded(pc.bytes ? pc.bytes : 1);
    HIPCHK(t.block.grow(total));
    hipError_t e = hipMemset(t.block, 0, total);                       // stamps 0 (epochs start at 1), padding boxes 0
    char* at = t.block;
    for (const piece& pc : pieces) {
        *pc.dst = call_memory::take(at, pc.bytes ? pc.bytes : 1);
        if (e == hipSuccess && pc.src && pc.bytes) e = hipMemcpy(*pc.dst, pc.src, pc.bytes, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { t.block.adopt(nullptr, 0); HIPCHK(e); }
    rt_refit_params& p = t.p;
    memset(&p, 0, sizeof(p));
    p.n_materials = s->dev.n_materials;
    p.spheres = const_cast<rt_sphere*>(s->dev.spheres); p.instances = const_cast<rt_instance*>(s->dev.instances);
    p.quads = const_cast<rt_quad*>(s->dev.quads); p.boxes = const_cast<rt_box*>(s->dev.boxes); p.n_boxes = s->n_boxes;
    p.n_leaves = m; p.n_slots = slots;
    p.leaf_solid = d_lq; p.leaf_node_ref = d_lr; p.leaf_node_walk = d_lw;
    p.box_lo = d_lo; p.box_hi = d_hi;
    p.tier_lo = const_cast<float4*>(s->dev.leaf_lo); p.tier_hi = const_cast<float4*>(s->dev.leaf_hi);
    p.nodes_ref = const_cast<rt_node*>(s->dev.nodes_ref);
    p.nodes_walk = own_walk ? const_cast<rt_node*>(s->dev.nodes) : nullptr;
    p.slot_box = tier ? const_cast<float*>(s->dev.slot_ranges) : d_slot;
    p.slot_abs = d_abs;
    p.jobs = d_jobs; p.n_jobs = (int32_t)jobs.size();
    p.result = d_result;
    t.ready = true;
    return RT_OK;
}

// The launches of an update whose records and indices are in place, the read-back of the bound and the flag, and the cost half
// of the calibration when asked for (as rt_scene_set_camera)
rt_status run_refit(rt_scene* s, const rt_refit_params& p, int kind, hipStream_t stream, int recalibrate, bool& refused) {
    HIPCHK(hipMemsetAsync(p.result, 0, 16, stream));
    HIPCHK(rt_launch_refit(p, kind, stream));
    float result[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    HIPCHK(hipMemcpyAsync(result, p.result, sizeof(result), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int c = 0; c < 3; ++c) s->dev.bound[c] = result[c];
    uint32_t flag = 0;
    memcpy(&flag, &result[3], 4);
    refused = flag != 0;
    if (recalibrate) RT_TRY(recalibrate_cost(s));
    return RT_OK;
}

// What an update of one kind names: its entry, the size of a record and the tail of the refusal of a device-resident record.
struct update_words { const char* entry; size_t record_bytes; const char* refused; };
const update_words UPDATE_WORDS[rt_refit::KINDS] = {
    {"rt_scene_update_spheres", sizeof(rt_sphere), "a non-finite field or a material out of range"},
    {"rt_scene_update_instances", sizeof(rt_instance), "a non-finite field, flags outside 1..3 or a child other than the scene's"},
    {"rt_scene_update_quads", sizeof(rt_quad), "a non-finite field or a material out of range"},
};

// The one body of rt_scene_update_spheres, _instances and _quads.  `why` is the answer of the kind's host check (rt_refit_host.h),
// made before any HIP call; n the scene's count of the kind.  The scene holds one copy of every record array (s->dev.spheres,
// .instances, .quads, .boxes), which every kernel reads through its scene view: the tier arrays hold references to the quads and
// boxes (lo.w / hi.w), the staged kernels copy at launch time, nothing is staged from the instances.  What rt_scene_create derives
// from quad records lives inside those arrays (pad0, bit 30 of first_quad) and follows the update there.
extern "C++" template <class Update>
rt_status update_records(rt_scene* s, int kind, const Update* u, const std::string& why, int32_t n, int on_device, int recalibrate, void* stream_v) {
    const update_words& w = UPDATE_WORDS[kind];
    const std::string who = std::string(w.entry) + ": ";
    if (!why.empty()) return invalid((who + why).c_str());
    if (u->count == 0) return RT_OK;
    RT_TRY(use_device(s->device));
    RT_TRY(build_refit_tables(s));
    rt_scene::refit_tables& t = s->refit;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const size_t bytes = (size_t)u->count * w.record_bytes;
    if (on_device) {
        const traced_ptr records[] = {{rt_refit::records_of(*u), bytes, rt_refit::NOUNS[kind].many, 4}};
        RT_TRY(check_trace_ptrs(records, s->device, w.entry));
    }
    if (s->frame_pending) RT_TRY(rt_frame_finish(s, nullptr));
    ++s->scene_epoch;                                // the cost map: as rt_scene_set_camera
    if (recalibrate) s->cost_map.valid = false;
    rt_refit_params p = t.p;
    p.count = u->count; p.first = u->first;
    p.stamp = t.stamp[kind];
    if (++t.epoch[kind] == 0) { HIPCHK(hipMemsetAsync(p.stamp, 0, (size_t)n * 4, stream)); t.epoch[kind] = 1; }
    p.epoch = t.epoch[kind];
    if (u->indices) {
        HIPCHK(t.d_indices.grow((size_t)u->count));
        HIPCHK(hipMemcpyAsync(t.d_indices, u->indices, (size_t)u->count * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        p.indices = t.d_indices;
    }
    if (on_device) p.records = rt_refit::records_of(*u);
    else {
        HIPCHK(t.d_records.grow(bytes));
        HIPCHK(hipMemcpyAsync(t.d_records, rt_refit::records_of(*u), bytes, hipMemcpyHostToDevice, stream));
        p.records = t.d_records;
    }
    bool refused = false;
    RT_TRY(run_refit(s, p, kind, stream, recalibrate, refused));
    if (refused) return invalid((who + "a device-resident record has " + w.refused + "; it was not stored, every other record was").c_str());
    return RT_OK;
}

// rt_scene_get_spheres, _instances, _quads: the scene's n records of the kind, as they stand on the device
extern "C++" template <class Record>
rt_status get_records(const rt_scene* s, int kind, const char* entry, const Record* records, int32_t n, Record* out, int32_t cap) {
    const std::string who = std::string(entry) + ": ";
    if (!out) return invalid((who + "null output pointer").c_str());
    if (cap < n) return invalid((who + "cap is below the scene's " + rt_refit::NOUNS[kind].one + " count").c_str());
    RT_TRY(use_device(s->device));
    if (n) HIPCHK(hipMemcpy(out, records, (size_t)n * sizeof(Record), hipMemcpyDeviceToHost));
    return RT_OK;
}

// The one body of rt_refit_nodes, rt_refit_instances and rt_refit_quads, after the kind's check has passed: the description's
// records of the kind with the update's in place (`changed`, which is one of the three arrays handed to the refit), the nodes refit.
extern "C++" template <class Update, class Record>
void restate(const rt_scene_desc* d, int kind, const Update* u, std::vector<Record>& changed, const rt_sphere* spheres, const rt_instance* instances,
             const rt_quad* quads, rt_node* nodes_out, Record* records_out) {
    std::vector<char> moved(changed.size(), 0);
    for (int32_t k = 0; k < u->count; ++k) {
        const int32_t i = u->indices ? u->indices[k] : u->first + k;
        changed[(size_t)i] = rt_refit::records_of(*u)[k];
        moved[(size_t)i] = 1;
    }
    if (nodes_out) {
        std::vector<rt_node> nodes(d->nodes, d->nodes + d->n_nodes);
        rt_refit::refit_nodes(nodes.data(), d, spheres, instances, quads, kind, moved);
        if (d->n_nodes) memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(rt_node));
    }
    if (records_out && !changed.empty()) memcpy(records_out, changed.data(), changed.size() * sizeof(Record));
}
rt_status validate_desc(const rt_scene_desc* d) {
    rt_scene_plan::scene_class cls;
    const char* why = rt_scene_plan::validate(d, cls);
    return why ? invalid(why) : RT_OK;
}
}  // namespace

rt_status rt_scene_update_spheres(rt_scene* s, const rt_sphere_update* u, int spheres_on_device, int recalibrate, void* stream_v) {
    if (!s) return invalid("rt_scene_update_spheres: null scene");
    const std::string why = rt_refit::check_update(u, !spheres_on_device, s->dev.n_spheres, s->dev.n_materials, s->refit.instanced);
    return update_records(s, rt_refit::SPHERES, u, why, s->dev.n_spheres, spheres_on_device, recalibrate, stream_v);
}

rt_status rt_scene_update_instances(rt_scene* s, const rt_instance_update* u, int instances_on_device, int recalibrate, void* stream_v) {
    if (!s) return invalid("rt_scene_update_instances: null scene");
    const std::string why = rt_refit::check_instance_update(u, !instances_on_device, s->refit.inst_child.data(), s->n_instances);
    return update_records(s, rt_refit::INSTANCES, u, why, s->n_instances, instances_on_device, recalibrate, stream_v);
}

rt_status rt_scene_update_quads(rt_scene* s, const rt_quad_update* u, int quads_on_device, int recalibrate, void* stream_v) {
    if (!s) return invalid("rt_scene_update_quads: null scene");
    const std::string why = rt_refit::check_quad_update(u, !quads_on_device, s->n_quads, s->dev.n_materials);
    return update_records(s, rt_refit::QUADS, u, why, s->n_quads, quads_on_device, recalibrate, stream_v);
}

rt_status rt_scene_get_spheres(const rt_scene* s, rt_sphere* out, int32_t cap) {
    if (!s) return invalid("rt_scene_get_spheres: null scene");
    return get_records(s, rt_refit::SPHERES, "rt_scene_get_spheres", s->dev.spheres, s->dev.n_spheres, out, cap);
}

rt_status rt_scene_get_instances(const rt_scene* s, rt_instance* out, int32_t cap) {
    if (!s) return invalid("rt_scene_get_instances: null scene");
    return get_records(s, rt_refit::INSTANCES, "rt_scene_get_instances", s->dev.instances, s->n_instances, out, cap);
}

rt_status rt_scene_get_quads(const rt_scene* s, rt_quad* out, int32_t cap) {
    if (!s) return invalid("rt_scene_get_quads: null scene");
    RT_TRY(get_records(s, rt_refit::QUADS, "rt_scene_get_quads", s->dev.quads, s->n_quads, out, cap));
    for (int32_t i = 0; i < s->n_quads; ++i) out[i].pad0 = 0.0f;        // (the device keeps the axis code there)
    return RT_OK;
}

rt_status rt_refit_nodes(const rt_scene_desc* d, const rt_sphere_update* u, rt_node* nodes_out, rt_sphere* spheres_out) {
    RT_TRY(validate_desc(d));
    const std::string why = rt_refit::check_update(u, true, d->n_spheres, d->n_materials, rt_refit::instanced_spheres(d->instances, d->n_instances, d->n_spheres));
    if (!why.empty()) return invalid(("rt_refit_nodes: " + why).c_str());
    std::vector<rt_sphere> spheres(d->spheres, d->spheres + d->n_spheres);
    restate(d, rt_refit::SPHERES, u, spheres, spheres.data(), d->instances, d->quads, nodes_out, spheres_out);
    return RT_OK;
}

rt_status rt_refit_instances(const rt_scene_desc* d, const rt_instance_update* u, rt_node* nodes_out, rt_instance* instances_out) {
    RT_TRY(validate_desc(d));
    std::vector<int32_t> children;
    for (int i = 0; i < d->n_instances; ++i) children.push_back(d->instances[i].child);
    const std::string why = rt_refit::check_instance_update(u, true, children.data(), d->n_instances);
    if (!why.empty()) return invalid(("rt_refit_instances: " + why).c_str());
    std::vector<rt_instance> instances(d->instances, d->instances + d->n_instances);
    restate(d, rt_refit::INSTANCES, u, instances, d->spheres, instances.data(), d->quads, nodes_out, instances_out);
    return RT_OK;
}

rt_status rt_refit_quads(const rt_scene_desc* d, const rt_quad_update* u, rt_node* nodes_out, rt_quad* quads_out) {
    RT_TRY(validate_desc(d));
    const std::string why = rt_refit::check_quad_update(u, true, d->n_quads, d->n_materials);
    if (!why.empty()) return invalid(("rt_refit_quads: " + why).c_str());
    std::vector<rt_quad> quads(d->quads, d->quads + d->n_quads);
    restate(d, rt_refit::QUADS, u, quads, d->spheres, d->instances, quads.data(), nodes_out, quads_out);
    return RT_OK;
}

rt_status rt_trace_rays(rt_scene* s, const rt_ray_batch* b, void* stream_v, int blocking) {
    // argument checks: no HIP call and no look at the scene before they pass
    if (!b) return invalid("rt_trace_rays: null batch");
    if (b->n < 0) return invalid("rt_trace_rays: negative ray count");
    if (!std::isfinite(b->tmin)) return invalid("rt_trace_rays: tmin is not finite");
    if (b->mode != RT_TRACE_CLOSEST && b->mode != RT_TRACE_ANY) return invalid("rt_trace_rays: unknown mode");
    if (!b->origins || !b->directions) return invalid("rt_trace_rays: null origins or directions");
    const bool record = b->point_out || b->normal_out || b->uv_out || b->mat_out;
    if (b->mode == RT_TRACE_ANY) {
        if (b->t_out || b->prim_out || b->inst_out || record) return invalid("rt_trace_rays: ANY mode takes hit_out only");
        if (!b->hit_out) return invalid("rt_trace_rays: ANY mode needs hit_out");
    } else {
        if (b->hit_out) return invalid("rt_trace_rays: CLOSEST mode does not take hit_out");
        if (!b->t_out || !b->prim_out) return invalid("rt_trace_rays: CLOSEST mode needs t_out and prim_out");
    }
    if (!s) return invalid("rt_trace_rays: null scene");
    if (b->n == 0) return RT_OK;
    RT_TRY(use_device(s->device));
    const size_t n = (size_t)b->n, f = sizeof(float), i = sizeof(int32_t);
    const traced_ptr ptrs[] = {
        {b->origins, 3 * n * f, "origins", 4}, {b->directions, 3 * n * f, "directions", 4}, {b->times, n * f, "times", 4}, {b->tmax, n * f, "tmax", 4},
        {b->t_out, n * f, "t_out", 4}, {b->prim_out, n * i, "prim_out", 4}, {b->inst_out, n * i, "inst_out", 4}, {b->point_out, 3 * n * f, "point_out", 4},
        {b->normal_out, 3 * n * f, "normal_out", 4}, {b->uv_out, 2 * n * f, "uv_out", 4}, {b->mat_out, n * i, "mat_out", 4}, {b->hit_out, n, "hit_out", 4}};
    RT_TRY(check_trace_ptrs(ptrs, s->device, "rt_trace_rays"));

    rt_trace_params tp;
    memset(&tp, 0, sizeof(tp));
    tp.n = b->n; tp.origins = b->origins; tp.directions = b->directions; tp.times = b->times; tp.tmax = b->tmax; tp.tmin = b->tmin;
    tp.record = record ? 1 : 0;
    tp.t_out = b->t_out; tp.prim_out = b->prim_out; tp.inst_out = b->inst_out;
    tp.point_out = b->point_out; tp.normal_out = b->normal_out; tp.uv_out = b->uv_out; tp.mat_out = b->mat_out;
    tp.hit_out = b->hit_out;

    // the node array: the walk array (the render's) or the reference's full tree; both carry the same leaves
    rt_scene_dev sd = s->dev;
    if (g_opt.trace_tree == 0) { sd.nodes = sd.nodes_ref; sd.n_nodes = sd.n_nodes_ref; }
    const bool any = b->mode == RT_TRACE_ANY;
    resident_plan plan;
    RT_TRY(plan_resident(s, (size_t)sd.n_nodes * sizeof(rt_node), g_opt.trace_lds, (b->n + RT_TRACE_THREADS - 1) / RT_TRACE_THREADS,
                         [&](int m, size_t lds, int* per_cu) { return rt_trace_occupancy(s->spheres_only, m, any, record, lds, per_cu); }, plan));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    HIPCHK(rt_launch_trace(s->spheres_only, plan.lds_mode, sd, tp, plan.grid, plan.lds, stream));
    if (blocking) HIPCHK(hipStreamSynchronize(stream));
    return RT_OK;
}

rt_status rt_radiance_rays(rt_scene* s, const rt_radiance_batch* b, void* stream_v, int blocking) {
    // argument checks: no HIP call and no look at the scene before they pass
    if (!b) return invalid("rt_radiance_rays: null batch");
    if (b->n < 0) return invalid("rt_radiance_rays: negative ray count");
    if (b->ns < 1 || b->ns > (1 << 20)) return invalid("rt_radiance_rays: ns outside 1 .. 1 << 20");
    if (!b->origins || !b->directions) return invalid("rt_radiance_rays: null origins or directions");
    if (!b->rgb_out) return invalid("rt_radiance_rays: null rgb_out");
    if (!s) return invalid("rt_radiance_rays: null scene");
    if (b->n == 0) return RT_OK;
    RT_TRY(use_device(s->device));
    const size_t n = (size_t)b->n, f = sizeof(float);
    const traced_ptr ptrs[] = {
        {b->origins, 3 * n * f, "origins", 4}, {b->directions, 3 * n * f, "directions", 4}, {b->times, n * f, "times", 4},
        {b->seeds, n * sizeof(uint64_t), "seeds", 8}, {b->rgb_out, 3 * n * f, "rgb_out", 4}, {b->rays_out, n * sizeof(uint32_t), "rays_out", 4}};
    RT_TRY(check_trace_ptrs(ptrs, s->device, "rt_radiance_rays"));

    rt_radiance_params rp;
    memset(&rp, 0, sizeof(rp));
    rp.n = b->n; rp.origins = b->origins; rp.directions = b->directions; rp.times = b->times; rp.seeds = b->seeds;
    rp.seed_base = b->seed_base; rp.ns = b->ns; rp.use_gradient_bg = b->use_gradient_bg;
    for (int k = 0; k < 3; ++k) rp.background[k] = b->background[k];
    rp.rgb_out = b->rgb_out; rp.rays_out = b->rays_out;

    const rt_scene_dev& sd = s->dev;   // the walk array
    resident_plan plan;
    RT_TRY(plan_resident(s, (size_t)sd.n_nodes * sizeof(rt_node), g_opt.radiance_lds, (b->n + RT_RADIANCE_THREADS - 1) / RT_RADIANCE_THREADS,
                         [&](int m, size_t lds, int* per_cu) { return rt_radiance_occupancy(s->spheres_only, s->tex_level, m, lds, per_cu); }, plan));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    HIPCHK(rt_launch_radiance(s->spheres_only, s->tex_level, plan.lds_mode, sd, rp, plan.grid, plan.lds, stream));
    if (blocking) HIPCHK(hipStreamSynchronize(stream));
    return RT_OK;
}

// rt_render_aov (t null) and rt_render_aov_through (t non-null, checked by the caller for null): one body, `who` names the entry
// point in the texts of failed checks
static rt_status aov_impl(rt_scene* s, const rt_frame_desc* f, const rt_aov_desc* a, const rt_aov_through_desc* t, const char* who_c,
                          int buffers_on_device, void* stream_v, int blocking) {
    // argument checks: no HIP call and no look at the scene before they pass
    const std::string who(who_c);
    auto bad = [&](const char* why) { return invalid((who + ": " + why).c_str()); };
    if (!f) return bad("null frame description");
    if (!a) return bad("null output description");
    if (t) {
        if (t->max_bounces < 0 || t->max_bounces > 16) return bad("max_bounces must be in 0..16");
        if (!(std::isfinite(t->fuzz_limit) && t->fuzz_limit >= 0.f)) return bad("fuzz_limit must be finite and >= 0");
    }
    if (!a->albedo && !a->normal && !a->depth && !a->alpha && !a->prim && !a->inst && !a->mat && !(t && (t->through || t->bounces)))
        return bad("every output is null");
    frame_geometry g;
    RT_TRY(check_frame(who_c, f, true, RENDER_FRAME_TEXTS, g));
    if (!s) return bad("null scene");
    if (g.local_rows == 0) return RT_OK;
    RT_TRY(use_device(s->device));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);

    rt_aov_params ap;
    memset(&ap, 0, sizeof(ap));
    rt_aov_through_params tp;
    memset(&tp, 0, sizeof(tp));
    const size_t pixels = g.n_pixels;
    const size_t f1 = pixels * sizeof(float), i1 = pixels * sizeof(int32_t);
    struct out_buffer : call_buffer { void** slot; };   // ... and where its device pointer goes
    auto out = [](const void* p, size_t bytes, const char* what, const void* slot) { return out_buffer{{{p, bytes, what, 4}, BUF_OUTPUT}, (void**)slot}; };
    const out_buffer bufs[] = {out(a->albedo, 3 * f1, "albedo", &ap.albedo), out(a->normal, 3 * f1, "normal", &ap.normal), out(a->depth, f1, "depth", &ap.depth),
                               out(a->alpha, f1, "alpha", &ap.alpha), out(a->prim, i1, "prim", &ap.prim), out(a->inst, i1, "inst", &ap.inst),
                               out(a->mat, i1, "mat", &ap.mat), out(t ? t->through : nullptr, f1, "through", &tp.through),
                               out(t ? t->bounces : nullptr, i1, "bounces", &tp.bounces)};
    enum { N_BUFS = sizeof(bufs) / sizeof(bufs[0]) };
    if (buffers_on_device) RT_TRY(check_trace_ptrs(bufs, s->device, who_c));
    // host buffers are staged in one allocation of this call's own (no per-frame resource of rt_render is used)
    const void* dev[N_BUFS];
    for (int k = 0; k < N_BUFS; ++k) dev[k] = bufs[k].p;
    call_memory mem;
    mem.guard(stream);
    if (!buffers_on_device) RT_TRY(stage_buffers(mem, bufs, [&](int k) { return bufs[k].p != nullptr; }, dev));
    for (int k = 0; k < N_BUFS; ++k) *bufs[k].slot = const_cast<void*>(dev[k]);
    ap.seed_base = f->seed_base;
    ap.nx = f->nx; ap.ny = f->ny; ap.ns = f->ns;
    ap.use_gradient_bg = f->use_gradient_bg;
    for (int k = 0; k < 3; ++k) ap.background[k] = f->background[k];
    ap.tile_rows = f->tile_rows; ap.tile_first = f->tile_first; ap.tile_stride = f->tile_stride;
    ap.local_rows = g.local_rows;
    ap.tiles_x = g.tiles_x;
    ap.work_items = g.work_items;
    if (t) { tp.max_bounces = t->max_bounces; tp.fuzz_limit = t->fuzz_limit; }

    const rt_scene_dev& sd = s->dev;   // the walk array
    resident_plan plan;
    RT_TRY(plan_resident(s, (size_t)sd.n_nodes * sizeof(rt_node), t ? g_opt.aov_through_lds : g_opt.aov_lds,
                         ((long long)ap.work_items + RT_AOV_THREADS - 1) / RT_AOV_THREADS,
                         [&](int m, size_t lds, int* per_cu) {
                             return t ? rt_aov_through_occupancy(s->spheres_only, s->tex_level, m, lds, per_cu)
                                      : rt_aov_occupancy(s->spheres_only, s->tex_level, m, lds, per_cu);
                         }, plan));
    if (t) HIPCHK(rt_launch_aov_through(s->spheres_only, s->tex_level, plan.lds_mode, sd, ap, tp, plan.grid, plan.lds, stream));
    else HIPCHK(rt_launch_aov(s->spheres_only, s->tex_level, plan.lds_mode, sd, ap, plan.grid, plan.lds, stream));
    if (!buffers_on_device) RT_TRY(download_outputs(bufs, dev, stream));
    return mem.finish(blocking || !buffers_on_device);
}

rt_status rt_render_aov(rt_scene* s, const rt_frame_desc* f, const rt_aov_desc* a, int buffers_on_device, void* stream_v, int blocking) {
    return aov_impl(s, f, a, nullptr, "rt_render_aov", buffers_on_device, stream_v, blocking);
}

rt_status rt_render_aov_through(rt_scene* s, const rt_frame_desc* f, const rt_aov_desc* a, const rt_aov_through_desc* t, int buffers_on_device,
                                void* stream_v, int blocking) {
    if (!t) return invalid("rt_render_aov_through: null chain description");
    return aov_impl(s, f, a, t, "rt_render_aov_through", buffers_on_device, stream_v, blocking);
}

size_t rt_denoise_workspace_bytes(int32_t nx, int32_t ny) {
    if (nx < 1 || ny < 1 || (long long)nx * ny >= (1ll << 31)) return 0;
    const size_t image = ((size_t)nx * ny * sizeof(float4) + 255) & ~(size_t)255;
    return 3 * image;   // x_k, x_{k+1} and the guide records
}

// rt_denoise (vd null) and rt_denoise_variance (vd non-null, checked by the caller for null): one body, `who` names the entry
// point in the texts of failed checks
static rt_status denoise_impl(const rt_denoise_desc* d, const rt_denoise_variance_desc* vd, const char* who_c, int buffers_on_device, void* stream_v, int blocking) {
    // argument checks: no HIP call before they pass
    const std::string who(who_c);
    auto bad = [&](const char* why) { return invalid((who + ": " + why).c_str()); };
    if (!d) return bad("null description");
    if (d->nx < 1 || d->ny < 1) return bad("nx and ny must be positive");
    if ((long long)d->nx * d->ny >= (1ll << 31)) return bad("frame too large");
    if (d->iterations < 1 || d->iterations > 8) return bad("iterations must be in 1..8");
    if (d->normal_sharpness < 0 || d->normal_sharpness > 10) return bad("normal_sharpness must be in 0..10");
    auto in_range = [](float v) { return std::isfinite(v) && v >= 1e-6f && v <= 1e6f; };
    auto sigma_ok = [&](float v) { return v == 0.f || in_range(v); };
    if (!sigma_ok(d->sigma_depth)) return bad("sigma_depth must be 0 or in [1e-6, 1e6]");
    if (vd) {
        if (d->sigma_color != 0.f) return bad("sigma_color must be 0 (the variance factor replaces the colour factor)");
        if (!in_range(vd->sigma_variance)) return bad("sigma_variance must be in [1e-6, 1e6]");
        if (!(std::isfinite(vd->variance_floor) && vd->variance_floor > 0.f)) return bad("variance_floor must be finite and positive");
        if (!vd->variance) return bad("null variance");
    } else {
        if (!sigma_ok(d->sigma_color)) return bad("sigma_color must be 0 or in [1e-6, 1e6]");
        if (d->sigma_color > 0.f && !(std::isfinite(d->color_floor) && d->color_floor > 0.f)) return bad("color_floor must be finite and positive");
    }
    if (!d->color) return bad("null color");
    if (!d->out) return bad("null out");
    if (d->demodulate && !d->albedo) return bad("demodulate needs albedo");
    const size_t pixels = (size_t)d->nx * d->ny;
    const size_t ws_bytes = rt_denoise_workspace_bytes(d->nx, d->ny);
    const bool own_workspace = !buffers_on_device || !d->workspace;
    if (d->workspace && d->workspace_bytes < ws_bytes) return bad("workspace smaller than rt_denoise_workspace_bytes");
    enum { COLOR = 0, ALBEDO, NORMAL, DEPTH, OUT, WORKSPACE, VARIANCE, VARIANCE_OUT, N_BUFS };
    const size_t f1 = pixels * sizeof(float), f3 = 3 * f1;
    const call_buffer bufs[N_BUFS] = {{{d->color, f3, "color", 4}, BUF_INPUT}, {{d->albedo, f3, "albedo", 4}, BUF_INPUT}, {{d->normal, f3, "normal", 4}, BUF_INPUT},
                                      {{d->depth, f1, "depth", 4}, BUF_INPUT}, {{d->out, f3, "out", 4}, BUF_OUTPUT},
                                      {{own_workspace ? nullptr : d->workspace, ws_bytes, "workspace", 16}, BUF_WORKSPACE},
                                      {{vd ? vd->variance : nullptr, f1, "variance", 4}, BUF_INPUT}, {{vd ? vd->variance_out : nullptr, f1, "variance_out", 4}, BUF_OUTPUT}};
    // out may be exactly color; nothing else may share a byte with out, with variance_out or with the workspace
    for (int k = 0; k < N_BUFS; ++k) {
        if (k != OUT && share_a_byte(bufs[k], bufs[OUT]) && !(k == COLOR && d->out == d->color)) return bad("out overlaps another buffer (it may only be exactly color)");
        if (k != WORKSPACE && share_a_byte(bufs[k], bufs[WORKSPACE])) return bad("the workspace overlaps another buffer");
        if (k != VARIANCE_OUT && share_a_byte(bufs[k], bufs[VARIANCE_OUT])) return bad("variance_out overlaps another buffer");
    }
    RT_TRY(use_device(g_device));
    if (buffers_on_device) RT_TRY(check_trace_ptrs(bufs, g_device, who_c));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);

    const bool normal_on = d->normal && d->normal_sharpness > 0, depth_on = d->depth && d->sigma_depth > 0.f, color_on = d->sigma_color > 0.f;
    const bool guide = normal_on || depth_on;
    // one allocation of this call's own: the workspace when the caller gives none and, for host buffers, their device images
    const void* dev[N_BUFS];
    for (int k = 0; k < N_BUFS; ++k) dev[k] = bufs[k].p;
    call_memory mem;
    mem.guard(stream);
    char* ws = static_cast<char*>(d->workspace);
    auto staged_image = [&](int k) { return !buffers_on_device && bufs[k].p && !(k == OUT && d->out == d->color); };
    if (own_workspace) RT_TRY(stage_buffers(mem, bufs, staged_image, dev, ws_bytes, &ws));   // the workspace comes first
    if (!buffers_on_device) {
        if (d->out == d->color) dev[OUT] = dev[COLOR];
        RT_TRY(upload_inputs(bufs, staged_image, dev, stream));
    }
    const size_t image = ws_bytes / 3;
    float4* x[2] = {reinterpret_cast<float4*>(ws), reinterpret_cast<float4*>(ws + image)};
    rt_denoise_params dp;
    memset(&dp, 0, sizeof(dp));
    dp.color = static_cast<const float*>(dev[COLOR]); dp.albedo = d->demodulate ? static_cast<const float*>(dev[ALBEDO]) : nullptr;
    dp.normal = normal_on ? static_cast<const float*>(dev[NORMAL]) : nullptr; dp.depth = depth_on ? static_cast<const float*>(dev[DEPTH]) : nullptr;
    dp.out = static_cast<float*>(const_cast<void*>(dev[OUT]));
    dp.guide = reinterpret_cast<float4*>(ws + 2 * image);
    dp.nx = d->nx; dp.ny = d->ny;
    dp.tiles_x = (d->nx + RT_DENOISE_TILE - 1) / RT_DENOISE_TILE;
    dp.normal_sharpness = d->normal_sharpness; dp.demodulate = d->demodulate ? 1 : 0;
    dp.color_floor = d->color_floor; dp.sigma_depth = d->sigma_depth;
    dp.x_out = x[0];
    rt_denoise_variance_params dv;
    memset(&dv, 0, sizeof(dv));
    if (vd) {
        dv.variance = static_cast<const float*>(dev[VARIANCE]); dv.variance_out = static_cast<float*>(const_cast<void*>(dev[VARIANCE_OUT]));
        dv.sigma_variance = vd->sigma_variance; dv.variance_floor = vd->variance_floor;
        HIPCHK(rt_launch_denoise_pack_variance(dp, dv, guide, stream));
    } else {
        HIPCHK(rt_launch_denoise_pack(dp, guide, stream));
    }
    // staged or direct, per iteration: staging fetches (16 + 4 s)^2 / 256 records per pixel and array instead
    // of 25 -- 1.6, 2.3, 4 for s = 1, 2, 4 -- and at s = 8 (9 per pixel, 84 KiB: one workgroup per CU) no longer pays
    const int max_staged = g_opt.denoise_lds < 0 ? 4 : (g_opt.denoise_lds == 0 ? 0 : RT_DENOISE_MAX_STAGED_STEP);
    for (int k = 0; k < d->iterations; ++k) {
        dp.step = 1 << k;
        dp.sigma_color_k = d->sigma_color * (1.0f / (float)(1 << k));
        dp.x_in = x[k & 1]; dp.x_out = x[(k + 1) & 1];
        dp.last = k == d->iterations - 1;
        if (vd) HIPCHK(rt_launch_denoise_variance(normal_on, depth_on, dp.step <= max_staged, dp, dv, stream));
        else HIPCHK(rt_launch_denoise(normal_on, depth_on, color_on, dp.step <= max_staged, dp, stream));
    }
    if (!buffers_on_device) RT_TRY(download_outputs(bufs, dev, stream));
    return mem.finish(blocking || own_workspace);
}

rt_status rt_denoise(const rt_denoise_desc* d, int buffers_on_device, void* stream_v, int blocking) {
    return denoise_impl(d, nullptr, "rt_denoise", buffers_on_device, stream_v, blocking);
}

rt_status rt_denoise_variance(const rt_denoise_desc* d, const rt_denoise_variance_desc* vd, int buffers_on_device, void* stream_v, int blocking) {
    if (!vd) return invalid("rt_denoise_variance: null variance description");
    return denoise_impl(d, vd, "rt_denoise_variance", buffers_on_device, stream_v, blocking);
}

// ---- rt_upscale (include/rt_abi.h)
rt_status rt_upscale(const rt_upscale_desc* d, int buffers_on_device, void* stream_v, int blocking) {
    // argument checks: no HIP call before they pass
    const char* who = "rt_upscale";
    auto bad = [&](const char* why) { return invalid((std::string(who) + ": " + why).c_str()); };
    if (!d) return bad("null description");
    if (!d->color_lo) return bad("null color_lo");
    if (!d->out) return bad("null out");
    if (d->factor < 2 || d->factor > 8) return bad("factor must be in 2..8");
    if (d->nx < 1 || d->ny < 1 || d->nx % d->factor || d->ny % d->factor) return bad("nx and ny must be positive multiples of factor");
    if ((long long)d->nx * d->ny >= (1ll << 31)) return bad("frame too large");
    if (d->normal_sharpness < 0 || d->normal_sharpness > 10) return bad("normal_sharpness must be in 0..10");
    if (!(d->sigma_depth == 0.f || (std::isfinite(d->sigma_depth) && d->sigma_depth >= 1e-6f && d->sigma_depth <= 1e6f)))
        return bad("sigma_depth must be 0 or in [1e-6, 1e6]");
    if (!(std::isfinite(d->min_weight) && d->min_weight >= 0.f && d->min_weight <= 1.f)) return bad("min_weight must be in [0, 1]");
    if (!d->normal != !d->normal_lo) return bad("normal and normal_lo must both be given or both be null");
    if (!d->depth != !d->depth_lo) return bad("depth and depth_lo must both be given or both be null");
    if (d->demodulate && !(d->albedo_lo && d->albedo)) return bad("demodulate needs albedo_lo and albedo");
    const int lx = d->nx / d->factor, ly = d->ny / d->factor;
    const size_t pixels = (size_t)d->nx * d->ny, coarse = (size_t)lx * ly;
    enum { COLOR_LO = 0, ALBEDO_LO, NORMAL_LO, DEPTH_LO, ALBEDO, NORMAL, DEPTH, OUT, WEIGHT_OUT, N_BUFS };
    const size_t c1 = coarse * sizeof(float), c3 = 3 * c1, f1 = pixels * sizeof(float), f3 = 3 * f1;
    const call_buffer bufs[N_BUFS] = {{{d->color_lo, c3, "color_lo", 4}, BUF_INPUT}, {{d->albedo_lo, c3, "albedo_lo", 4}, BUF_INPUT},
                                      {{d->normal_lo, c3, "normal_lo", 4}, BUF_INPUT}, {{d->depth_lo, c1, "depth_lo", 4}, BUF_INPUT},
                                      {{d->albedo, f3, "albedo", 4}, BUF_INPUT}, {{d->normal, f3, "normal", 4}, BUF_INPUT}, {{d->depth, f1, "depth", 4}, BUF_INPUT},
                                      {{d->out, f3, "out", 4}, BUF_OUTPUT}, {{d->weight_out, f1, "weight_out", 4}, BUF_OUTPUT}};
    for (int k = 0; k < N_BUFS; ++k) {   // nothing may share a byte with out or with weight_out
        if (k != OUT && share_a_byte(bufs[k], bufs[OUT])) return bad("out overlaps another buffer");
        if (k != WEIGHT_OUT && share_a_byte(bufs[k], bufs[WEIGHT_OUT])) return bad("weight_out overlaps another buffer");
    }
    RT_TRY(use_device(g_device));
    if (buffers_on_device) RT_TRY(check_trace_ptrs(bufs, g_device, who));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);

    const bool normal_on = d->normal && d->normal_sharpness > 0, depth_on = d->depth && d->sigma_depth > 0.f;
    // host buffers are staged in one allocation of this call's own
    const void* dev[N_BUFS];
    for (int k = 0; k < N_BUFS; ++k) dev[k] = bufs[k].p;
    call_memory mem;
    mem.guard(stream);
    if (!buffers_on_device) {
        auto given = [&](int k) { return bufs[k].p != nullptr; };
        RT_TRY(stage_buffers(mem, bufs, given, dev));
        RT_TRY(upload_inputs(bufs, given, dev, stream));
    }
    auto in = [&](int k, bool used) { return used ? static_cast<const float*>(dev[k]) : nullptr; };
    rt_upscale_params up;
    memset(&up, 0, sizeof(up));
    up.color_lo = in(COLOR_LO, true);
    up.albedo_lo = in(ALBEDO_LO, d->demodulate != 0); up.albedo = in(ALBEDO, d->demodulate != 0);
    up.normal_lo = in(NORMAL_LO, normal_on); up.normal = in(NORMAL, normal_on);
    up.depth_lo = in(DEPTH_LO, depth_on); up.depth = in(DEPTH, depth_on);
    up.out = static_cast<float*>(const_cast<void*>(dev[OUT]));
    up.weight_out = static_cast<float*>(const_cast<void*>(dev[WEIGHT_OUT]));
    up.nx = d->nx; up.ny = d->ny; up.lx = lx; up.ly = ly; up.factor = d->factor;
    up.tiles_x = (d->nx + RT_DENOISE_TILE - 1) / RT_DENOISE_TILE;
    up.normal_sharpness = d->normal_sharpness; up.demodulate = d->demodulate ? 1 : 0;
    up.sigma_depth = d->sigma_depth; up.min_weight = d->min_weight;
    // staged or direct: auto is staged
    HIPCHK(rt_launch_upscale(normal_on, depth_on, g_opt.upscale_lds != 0, up, stream));
    if (!buffers_on_device) RT_TRY(download_outputs(bufs, dev, stream));
    return mem.finish(blocking || !buffers_on_device);
}

// ---- rt_reproject (include/rt_abi.h)
// The inverse of the previous camera's (A, H, V) basis, in double from its float fields, one rounding per written operation
// (the library is built with -ffp-contract=off, which this function's contract needs: no product may fuse into a sum).
rt_status rt_reproject_matrix(const rt_camera* prev, float m[9]) {
    if (!prev) return invalid("rt_reproject_matrix: null camera");
    if (!m) return invalid("rt_reproject_matrix: null output pointer");
    double A[3], H[3], V[3];
    for (int c = 0; c < 3; ++c) {
        A[c] = (double)prev->lower_left_corner[c] - (double)prev->origin[c];
        H[c] = (double)prev->horizontal[c];
        V[c] = (double)prev->vertical[c];
    }
    auto cross = [](const double* x, const double* y, double* out) {
        out[0] = x[1] * y[2] - x[2] * y[1];
        out[1] = x[2] * y[0] - x[0] * y[2];
        out[2] = x[0] * y[1] - x[1] * y[0];
    };
    double r[3][3];
    cross(H, V, r[0]);
    cross(V, A, r[1]);
    cross(A, H, r[2]);
    const double D = (A[0] * r[0][0] + A[1] * r[0][1]) + A[2] * r[0][2];
    if (D == 0.0) return invalid("rt_reproject_matrix: the camera's basis is singular (D == 0)");
    float out[9];
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) {
            out[3 * k + c] = (float)(r[k][c] / D);
            if (!std::isfinite(out[3 * k + c])) return invalid("rt_reproject_matrix: the matrix is not finite");
        }
    memcpy(m, out, sizeof(out));
    return RT_OK;
}

namespace {
// rt_reproject (m == null), rt_reproject_moving, rt_reproject_instances (im != null, with m) and rt_reproject_quads (qm != null, with
// both): the checks, the staging of host buffers and the parameter block are one
rt_status reproject_impl(const rt_reproject_desc* d, const rt_reproject_motion_desc* m, const rt_reproject_instance_desc* im,
                         const rt_reproject_quad_desc* qm, const char* who, int buffers_on_device, void* stream_v, int blocking) {
    // argument checks: no HIP call before they pass
    auto bad = [&](const char* why) { return invalid((std::string(who) + ": " + why).c_str()); };
    if (!d) return bad("null description");
    if (d->nx < 1 || d->ny < 1) return bad("nx and ny must be positive");
    if ((long long)d->nx * d->ny >= (1ll << 31)) return bad("frame too large");
    if (!(d->alpha_min > 0.f && d->alpha_min <= 1.f)) return bad("alpha_min must be in (0, 1]");
    if (!(d->depth_tol >= 0.f && d->depth_tol <= 1.f)) return bad("depth_tol must be in [0, 1]");
    if (!(d->normal_min >= -1.f && d->normal_min <= 1.f)) return bad("normal_min must be in [-1, 1]");
    if (!(d->max_history >= 1.f && d->max_history <= 65536.f)) return bad("max_history must be in [1, 65536]");
    if (!d->color) return bad("null color");
    if (!d->depth) return bad("null depth");
    if (!d->alpha) return bad("null alpha");
    if (!d->out) return bad("null out");
    if (!d->out_len) return bad("null out_len");
    if (d->history) {
        if (!d->history_len || !d->prev_depth || !d->prev_alpha) return bad("history needs history_len, prev_depth and prev_alpha");
    } else if (d->history_len || d->prev_depth || d->prev_alpha) {
        return bad("history_len, prev_depth and prev_alpha need history");
    }
    // one record table of both frames: the count's range, then both tables where it is positive.  `counts` is the subject of the
    // range messages and `other` a second count they cover (the sphere tables' are shared with n_media)
    auto check_table = [&](const std::string& counts, const std::string& name, int n, int other, const void* cur, const void* prev) -> rt_status {
        if (n < 0 || other < 0) return bad((counts + " must not be negative").c_str());
        if (n >= (1 << 28) || other >= (1 << 28)) return bad((counts + " must be below 2^28").c_str());
        if (n > 0 && (!cur || !prev)) return bad(("n_" + name + " > 0 needs " + name + " and prev_" + name).c_str());
        return RT_OK;
    };
    if (m) {
        if (!d->prim || !d->prev_prim) return bad("prim and prev_prim are required: they say which sphere a pixel shows");
        RT_TRY(check_table("n_spheres and n_media", "spheres", m->n_spheres, m->n_media, m->spheres, m->prev_spheres));
        if (m->n_media > 0 && !m->media) return bad("n_media > 0 needs media");
        if (!std::isfinite(m->time) || !std::isfinite(m->prev_time)) return bad("time and prev_time must be finite");
    }
    if (im) {
        if (!im->inst) return bad("null inst: it says which instance a pixel shows");
        if (d->history ? !im->prev_inst : im->prev_inst != nullptr) return bad("prev_inst must be non-null exactly when history is");
        RT_TRY(check_table("n_instances", "instances", im->n_instances, 0, im->instances, im->prev_instances));
    }
    if (qm) RT_TRY(check_table("n_quads", "quads", qm->n_quads, 0, qm->quads, qm->prev_quads));
    rt_reproject_params rp;
    memset(&rp, 0, sizeof(rp));
    if (rt_reproject_matrix(&d->prev, rp.m) != RT_OK) return bad("prev: the camera's basis is singular or its inverse is not finite");
    const size_t pixels = (size_t)d->nx * d->ny;
    enum { COLOR = 0, DEPTH, ALPHA, NORMAL, PRIM, HISTORY, HISTORY_LEN, PREV_DEPTH, PREV_ALPHA, PREV_NORMAL, PREV_PRIM, OUT, OUT_LEN, MOTION,
           SPHERES, PREV_SPHERES, MEDIA,            // the three tables: rt_reproject_moving and up, inputs behind the outputs
           INSTANCES, PREV_INSTANCES, INST, PREV_INST,   // rt_reproject_instances and up
           QUADS, PREV_QUADS, N_BUFS };                  // rt_reproject_quads only
    const size_t f1 = pixels * sizeof(float), f3 = 3 * f1;
    const size_t sphere_bytes = m ? (size_t)m->n_spheres * sizeof(rt_sphere) : 0, medium_bytes = m ? (size_t)m->n_media * sizeof(rt_medium) : 0;
    const size_t instance_bytes = im ? (size_t)im->n_instances * sizeof(rt_instance) : 0, quad_bytes = qm ? (size_t)qm->n_quads * sizeof(rt_quad) : 0;
    const call_buffer bufs[N_BUFS] = {{{d->color, f3, "color", 4}, BUF_INPUT}, {{d->depth, f1, "depth", 4}, BUF_INPUT}, {{d->alpha, f1, "alpha", 4}, BUF_INPUT},
                                      {{d->normal, f3, "normal", 4}, BUF_INPUT}, {{d->prim, f1, "prim", 4}, BUF_INPUT}, {{d->history, f3, "history", 4}, BUF_INPUT},
                                      {{d->history_len, f1, "history_len", 4}, BUF_INPUT}, {{d->prev_depth, f1, "prev_depth", 4}, BUF_INPUT},
                                      {{d->prev_alpha, f1, "prev_alpha", 4}, BUF_INPUT}, {{d->prev_normal, f3, "prev_normal", 4}, BUF_INPUT},
                                      {{d->prev_prim, f1, "prev_prim", 4}, BUF_INPUT}, {{d->out, f3, "out", 4}, BUF_OUTPUT}, {{d->out_len, f1, "out_len", 4}, BUF_OUTPUT},
                                      {{d->motion, 2 * f1, "motion", 4}, BUF_OUTPUT},
                                      {{sphere_bytes ? m->spheres : nullptr, sphere_bytes, "spheres", 4}, BUF_INPUT},
                                      {{sphere_bytes ? m->prev_spheres : nullptr, sphere_bytes, "prev_spheres", 4}, BUF_INPUT},
                                      {{medium_bytes ? m->media : nullptr, medium_bytes, "media", 4}, BUF_INPUT},
                                      {{instance_bytes ? im->instances : nullptr, instance_bytes, "instances", 4}, BUF_INPUT},
                                      {{instance_bytes ? im->prev_instances : nullptr, instance_bytes, "prev_instances", 4}, BUF_INPUT},
                                      {{im ? im->inst : nullptr, f1, "inst", 4}, BUF_INPUT}, {{im ? im->prev_inst : nullptr, f1, "prev_inst", 4}, BUF_INPUT},
                                      {{quad_bytes ? qm->quads : nullptr, quad_bytes, "quads", 4}, BUF_INPUT},
                                      {{quad_bytes ? qm->prev_quads : nullptr, quad_bytes, "prev_quads", 4}, BUF_INPUT}};
    for (int o = OUT; o <= MOTION; ++o)     // an output shares no byte with any other buffer
        for (int k = 0; k < N_BUFS; ++k)
            if (k != o && share_a_byte(bufs[o], bufs[k])) return bad((std::string(bufs[o].what) + " overlaps " + bufs[k].what).c_str());
    RT_TRY(use_device(g_device));
    if (buffers_on_device) RT_TRY(check_trace_ptrs(bufs, g_device, who));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);

    // (without a history no tap is read: the tests on taps are then off whatever guides were given)
    const bool normals_on = d->history && d->normal && d->prev_normal, ids_on = m || (d->history && d->prim && d->prev_prim), motion_on = d->motion != nullptr;
    auto used = [&](int k) {   // what the kernel reads or writes
        if (!bufs[k].p) return false;
        if (k == NORMAL || k == PREV_NORMAL) return normals_on;
        if (k == PRIM) return ids_on;
        if (k == PREV_PRIM) return ids_on && d->history;
        return true;
    };
    const void* dev[N_BUFS];
    for (int k = 0; k < N_BUFS; ++k) dev[k] = used(k) ? bufs[k].p : nullptr;
    call_memory mem;
    mem.guard(stream);
    if (!buffers_on_device) {   // host buffers: their device images in one allocation of this call's own
        RT_TRY(stage_buffers(mem, bufs, used, dev));
        RT_TRY(upload_inputs(bufs, used, dev, stream));
    }
    auto fptr = [&](int k) { return static_cast<const float*>(dev[k]); };
    auto iptr = [&](int k) { return static_cast<const int32_t*>(dev[k]); };
    rp.color = fptr(COLOR); rp.depth = fptr(DEPTH); rp.alpha = fptr(ALPHA); rp.normal = fptr(NORMAL); rp.prim = iptr(PRIM);
    rp.history = fptr(HISTORY); rp.history_len = fptr(HISTORY_LEN); rp.prev_depth = fptr(PREV_DEPTH); rp.prev_alpha = fptr(PREV_ALPHA);
    rp.prev_normal = fptr(PREV_NORMAL); rp.prev_prim = iptr(PREV_PRIM);
    rp.out = const_cast<float*>(fptr(OUT)); rp.out_len = const_cast<float*>(fptr(OUT_LEN)); rp.motion = const_cast<float*>(fptr(MOTION));
    rp.nx = d->nx; rp.ny = d->ny;
    rp.tiles_x = (d->nx + RT_REPROJECT_TILE - 1) / RT_REPROJECT_TILE;
    for (int c = 0; c < 3; ++c) {
        rp.origin[c] = d->cur.origin[c]; rp.lower_left[c] = d->cur.lower_left_corner[c];
        rp.horizontal[c] = d->cur.horizontal[c]; rp.vertical[c] = d->cur.vertical[c];
        rp.prev_origin[c] = d->prev.origin[c];
    }
    rp.alpha_min = d->alpha_min; rp.depth_tol = d->depth_tol; rp.normal_min = d->normal_min; rp.max_history = d->max_history;
    // the follow step's tables, filled as far as the entry's descriptions reach (dev[] and the byte counts are null and 0 beyond)
    rt_reproject_follow_quad_params qp;
    memset(&qp, 0, sizeof(qp));
    qp.spheres = static_cast<const rt_sphere*>(dev[SPHERES]); qp.prev_spheres = static_cast<const rt_sphere*>(dev[PREV_SPHERES]);
    qp.media = static_cast<const rt_medium*>(dev[MEDIA]);
    if (m) { qp.n_spheres = m->n_spheres; qp.n_media = m->n_media; qp.time = m->time; qp.prev_time = m->prev_time; }
    qp.instances = static_cast<const rt_instance*>(dev[INSTANCES]); qp.prev_instances = static_cast<const rt_instance*>(dev[PREV_INSTANCES]);
    qp.inst = iptr(INST); qp.prev_inst = iptr(PREV_INST);
    if (im) qp.n_instances = im->n_instances;
    qp.quads = static_cast<const rt_quad*>(dev[QUADS]); qp.prev_quads = static_cast<const rt_quad*>(dev[PREV_QUADS]);
    if (qm) qp.n_quads = qm->n_quads;
    const rt_reproject_form form = qm ? RT_REPROJECT_QUADS : im ? RT_REPROJECT_INSTANCES : m ? RT_REPROJECT_SPHERES : RT_REPROJECT_STATIC;
    HIPCHK(rt_launch_reproject(form, normals_on, ids_on, motion_on, rp, qp, stream));
    if (!buffers_on_device) RT_TRY(download_outputs(bufs, dev, stream));
    return mem.finish(blocking || !buffers_on_device);
}
}  // namespace

rt_status rt_reproject(const rt_reproject_desc* d, int buffers_on_device, void* stream_v, int blocking) {
    return reproject_impl(d, nullptr, nullptr, nullptr, "rt_reproject", buffers_on_device, stream_v, blocking);
}

rt_status rt_reproject_moving(const rt_reproject_desc* d, const rt_reproject_motion_desc* m, int buffers_on_device, void* stream_v, int blocking) {
    if (!m) return invalid("rt_reproject_moving: null motion description");
    return reproject_impl(d, m, nullptr, nullptr, "rt_reproject_moving", buffers_on_device, stream_v, blocking);
}

rt_status rt_reproject_instances(const rt_reproject_desc* d, const rt_reproject_motion_desc* m, const rt_reproject_instance_desc* im,
                                 int buffers_on_device, void* stream_v, int blocking) {
    if (!m) return invalid("rt_reproject_instances: null motion description");
    if (!im) return invalid("rt_reproject_instances: null instance description");
    return reproject_impl(d, m, im, nullptr, "rt_reproject_instances", buffers_on_device, stream_v, blocking);
}

rt_status rt_reproject_quads(const rt_reproject_desc* d, const rt_reproject_motion_desc* m, const rt_reproject_instance_desc* im,
                             const rt_reproject_quad_desc* qm, int buffers_on_device, void* stream_v, int blocking) {
    if (!m) return invalid("rt_reproject_quads: null motion description");
    if (!im) return invalid("rt_reproject_quads: null instance description");
    if (!qm) return invalid("rt_reproject_quads: null quad description");
    return reproject_impl(d, m, im, qm, "rt_reproject_quads", buffers_on_device, stream_v, blocking);
}

namespace {
// The main kernel's launch shape (plan_main_launch) under the current options, its stage quorums written to fp; a refusal is the
// caller's result.
rt_status main_launch_of(const plan_facts& c, int kernel, size_t n_pixels, rt_frame_params& fp, main_launch& ml) {
    const char* why = nullptr;
    if (plan_main_launch(c, g_opt, kernel, n_pixels, fp.work_items, ml, why) != RT_OK) return invalid(why);
    fp.shade_threshold = ml.shade_threshold; fp.newpath_threshold = ml.newpath_threshold;
    return RT_OK;
}
// kernel_variant and the launch shape as rt_stats reports them
void stats_of_launch(const plan_facts& c, const main_launch& ml, rt_stats& out) {
    out.kernel_variant = kernel_variant_of(c, ml);
    out.workgroups = (int)ml.grid.x; out.threads_per_group = (int)ml.block.x; out.lds_bytes = (int)ml.lds_bytes;
}

// The frame parameters every entry of the main kernel sets alike, for a frame of `ns` samples per pixel: the scene's counters, the
// frame description, the call's geometry and the scheduling knobs.  The caller adds fb, state_in / state_out, the sample window
// and store_parked, and the stage quorums of its main_launch.
void fill_frame_params(const rt_scene* s, const rt_frame_desc* f, const frame_geometry& g, int ns, rt_frame_params& fp) {
    memset(&fp, 0, sizeof(fp));
    fp.ray_counter = s->d_ray_counter;
    fp.work_counter = s->d_work_counter;
    fp.seed_base = f->seed_base;
    fp.nx = f->nx; fp.ny = f->ny; fp.ns = ns; fp.gamma = f->gamma;
    fp.background[0] = f->background[0]; fp.background[1] = f->background[1]; fp.background[2] = f->background[2];
    fp.use_gradient_bg = f->use_gradient_bg;
    fp.tile_rows = f->tile_rows; fp.tile_first = f->tile_first; fp.tile_stride = f->tile_stride;
    fp.local_rows = g.local_rows;
    fp.tiles_x = g.tiles_x;
    fp.work_items = g.work_items;
    fp.sparse_priority = g_opt.sparse_priority; fp.sparse_eager = g_opt.sparse_eager; fp.semi_priority = g_opt.semi_priority; fp.tier_priority = g_opt.tier_priority;
    fp.steps_per_trip = g_opt.steps_per_trip;
    fp.leaf_threshold = g_opt.leaf_threshold;
    fp.diel_threshold = g_opt.diel_threshold;
    fp.box_threshold = g_opt.box_threshold; fp.medium_threshold = g_opt.medium_threshold;
}

// the tier kernel of the scene's family
hipError_t launch_tier(const rt_scene* s, const rt_frame_params& fp, dim3 grid, size_t lds, hipStream_t stream) {
    return s->spheres_only ? rt_launch_tier_spheres(s->tex_level, s->dev, fp, grid, lds, stream)
                           : rt_launch_tier_general(s->tex_level, s->need_uv, s->dev, fp, grid, lds, stream);
}

enum { RT_HEAVY_CAP = 262144 };   // entries of the heavy list, unsorted and sorted

// The end of a synchronous frame (rt_render_adaptive, rt_render_variance), after its last enqueue: the wait, the time between
// ev_start and ev_stop, the ray counter, and the statistics, which stay in the scene as rt_render's do.  `passes` is what
// rt_stats::reserved reports for these entries.
rt_status finish_sync_frame(rt_scene* s, hipStream_t stream, int passes, rt_stats& out, rt_stats* stats) {
    HIPCHK(hipStreamSynchronize(stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, s->ev_start, s->ev_stop));
    unsigned long long rays = 0;
    HIPCHK(hipMemcpy(&rays, s->d_ray_counter, sizeof(rays), hipMemcpyDeviceToHost));
    out.ms_render = (double)ms;
    out.rays = rays;
    out.reserved = passes;
    s->pending_stats = out;
    if (stats) *stats = out;
    return RT_OK;
}

}  // namespace

static rt_status render_impl(rt_scene* s, const rt_frame_desc* f, float* fb, int fb_on_device, void* stream_v, int blocking, rt_stats* stats,
                             rt_progressive* win, int32_t win_begin, int32_t win_end);

rt_status rt_render(rt_scene* s, const rt_frame_desc* f, float* fb, int fb_on_device, void* stream_v, int blocking, rt_stats* stats) {
    return render_impl(s, f, fb, fb_on_device, stream_v, blocking, stats, nullptr, 0, 0);
}

rt_status rt_progressive_state_create(rt_scene* s, const rt_frame_desc* f, void** state) {
    if (!s || !f || !state) return invalid("null argument");
    *state = nullptr;
    RT_TRY(use_device(s->device));
    frame_geometry g;
    RT_TRY(check_frame(nullptr, f, false, STATE_FRAME_TEXTS, g));
    rt_progressive* p = new rt_progressive;
    p->scene = s; p->frame = *f; p->pixels = g.n_pixels; p->next_sample = 0;
    const hipError_t e = (hipError_t)p->d_state.grow(p->pixels ? p->pixels : 1);
    if (e != hipSuccess) { delete p; g_last_hip_error = (int)e; g_detail = "allocating the progressive state failed"; return RT_ERR_HIP; }
    *state = p;
    return RT_OK;
}

rt_status rt_progressive_state_destroy(rt_scene* s, void* state) {
    if (!state) return RT_OK;
    rt_progressive* p = static_cast<rt_progressive*>(state);
    if (s) (void)use_device(s->device);
    delete p;
    return RT_OK;
}

rt_status rt_render_window(rt_scene* s, const rt_frame_desc* f, float* fb, int fb_on_device, void* state, int32_t sample_begin, int32_t sample_end,
                           void* stream_v, int blocking, rt_stats* stats) {
    if (!s || !f || !fb || !state) return invalid("null argument");
    rt_progressive* p = static_cast<rt_progressive*>(state);
    if (p->scene != s) return invalid("rt_render_window: the state belongs to another scene");
    if (f->nx != p->frame.nx || f->ny != p->frame.ny || f->tile_rows != p->frame.tile_rows || f->tile_first != p->frame.tile_first ||
        f->tile_stride != p->frame.tile_stride || f->seed_base != p->frame.seed_base)
        return invalid("rt_render_window: the frame description differs from the one the state was created for");
    if (sample_begin != p->next_sample || sample_end <= sample_begin) return invalid("rt_render_window: windows must follow each other (sample_begin = the previous sample_end, 0 first)");
    const rt_status st = render_impl(s, f, fb, fb_on_device, stream_v, blocking, stats, p, sample_begin, sample_end);
    if (st == RT_OK) p->next_sample = sample_end;
    return st;
}

// ---- cost-aware schedule (staged kernel): the frame is split at sample boundaries.
// A pixel's samples are one sequential chain (one XORWOW stream) and the dearest pixels of a frame trace ~10x the
// mean number of rays, so the frame time is bounded by a few pixels' chains, not by throughput
// (tools/critical_chain.py: the worst 8 rows alone take as long as the whole frame).  Every part but the last parks
// each pixel at its end (XORWOW state, colour sum, rays traced: at a sample boundary no path is in flight, so that is
// the whole state), and every part is RANKED on what is known about the pixels' costs when it starts -- the
// calibration frame's prior for the first part, measured rays for the later ones:
//   * 8x8 tiles are served in descending cost (longest first);
//   * pixels far above the mean go to a short list, dearest first: tier 1 to the tier kernel (rt_kernel_tier.h, one
//     pixel per wave, on a stream of its own beside the main kernel), tier 2 to "sparse" main workgroups with a few live
//     lanes per wave at raised priority -- a lane's rays advance about twice as fast in a wave with few live lanes --,
//     tier 3 to ordinary lanes before any tile; ordinary waves skip listed pixels.
//   * the end of every part is handed over (rt_device.h, "tail hand-off"): when the tile queue is dry and only a few thousand
//     pixels are still in flight, the main kernel's lanes park them at their next sample boundary and a second launch of
//     the tier kernel, right behind the main kernel on the same stream, finishes them one per wave -- the last pixels of a
//     part are its cheapest ones started last, each still a chain of hundreds of rays at an ordinary lane's pace.
// The ranking runs on the device (rt_rank.hip) and leaves the tier sizes in device memory, so the whole frame is
// enqueued without a host round trip.  Scheduling only: every sample of every pixel is rendered exactly once, in
// its pixel's stream order; frames are bit-identical with and without it (tests sweep the knobs).
// What is decided -- the parts, what each is ranked on, the grids, the hand-off -- is plan_frame's (rt_frame_plan.h); the two
// functions below enqueue one part of a plan.

// One ranking: the cost prior of a fresh part into d_state and d_tile_cost, its sum into d_ray_counter[3] -- from the cost map,
// pixel for pixel, or from the calibration frame --, then three small kernels that order the tiles, list the heavy pixels and
// size the tiers for the launch described by `q` (which resumes every pixel from d_state).
static rt_status rank_part(rt_scene* s, const frame_plan& plan, const frame_part& part, rt_frame_params& q, hipStream_t stream) {
    if (part.ranked_on != RANK_MEASURED) {
        const bool from_map = part.ranked_on == RANK_MAP;
        rt_prior_params pp;
        memset(&pp, 0, sizeof(pp));
        pp.state = s->d_state; pp.tile_cost = s->d_tile_cost; pp.total = s->d_ray_counter + 3;
        pp.cal_cost = from_map ? s->cost_map.d : s->d_cal_cost; pp.cal_nx = s->cal_nx; pp.cal_ny = s->cal_ny;
        pp.nx = q.nx; pp.ny = q.ny; pp.local_rows = q.local_rows; pp.tiles_x = q.tiles_x;
        pp.tile_rows = q.tile_rows; pp.tile_first = q.tile_first; pp.tile_stride = q.tile_stride;
        HIPCHK(from_map ? rt_launch_prior_map(pp, stream) : rt_launch_prior(pp, stream));
    }
    const tier_sizes& e = plan.sizes;
    const unsigned block = plan.ml.block.x;
    rt_rank_params rp;
    memset(&rp, 0, sizeof(rp));
    rp.state = s->d_state; rp.tile_cost = s->d_tile_cost; rp.tile_order = s->d_tile_order;
    rp.ray_counter = part.ranked_on == RANK_MEASURED ? s->d_ray_counter : s->d_ray_counter + 3;   // the sum of the costs ranked on
    rp.heavy_list = s->d_heavy_list; rp.heavy_pixels = s->d_heavy_pixels; rp.info = s->d_rank;
    rp.n_pixels = (uint32_t)plan.ranked_pixels; rp.n_tiles = (uint32_t)plan.ranked_tiles; rp.heavy_cap = RT_HEAVY_CAP;
    rp.max_grid = plan.max_grid; rp.waves_per_wg = block / 64u;
    rp.normal_need = plan.normal_need;
    rp.sparse_stride = plan.sparse_stride;
    rp.semi_stride = plan.semi_stride;
    rp.sparse_percent = e.sparse_percent;
    rp.sparse_work_percent = e.work_percent;
    rp.tier_possible = plan.tier_possible ? 1 : 0;
    rp.tier1_pixels = e.tier1_pixels; rp.tier1_depth = e.tier1_depth;
    rp.tier_wgs_cap = (int32_t)plan.tier_grid; rp.tier_waves_per_main_wg = plan.tier_waves_per_main_wg;
    rp.nx = q.nx; rp.smooth_percent = plan.smooth_percent;
    rp.heavy_factor = (float)e.heavy_factor / 10.0f; rp.sparse_factor = (float)e.sparse_factor / 10.0f; rp.tier1_factor = (float)e.tier1_factor / 10.0f;
    HIPCHK(rt_launch_rank(rp, stream));
    q.tile_order = s->d_tile_order; q.heavy_pixels = s->d_heavy_pixels; q.rank = s->d_rank;
    return RT_OK;
}

// Part `k` of the frame: its ranking, the tier kernel (ranked parts of scenes that have tier data) on its own stream, forked from
// and joined to the caller's stream by events, the main kernel, and the tail.  `fp`: what the frame's parts share; `state`: where
// its pixels park (the scene's d_state, a progressive window's own).
static rt_status launch_part(rt_scene* s, const frame_plan& plan, int k, const rt_frame_params& fp, rt_pixel_state* state, hipStream_t stream) {
    const frame_part& part = plan.parts[k];
    const bool last = k + 1 == plan.n_parts;
    const size_t tier_lds = plan.room.lds;
    rt_frame_params q = fp;
    q.sample_begin = part.sample_begin; q.sample_end = part.sample_end; q.fresh = part.fresh ? 1 : 0;
    q.state_in = part.reads_state ? state : nullptr; q.state_out = part.parks_state ? state : nullptr;
    q.tile_cost = part.writes_tile_cost ? s->d_tile_cost : nullptr;
    if (last && plan.cost_out) q.cost_out = s->cost_map.d;
    if (part.tail) {
        q.handoff_queue = s->d_handoff; q.handoff_cap = (uint32_t)plan.handoff_capacity; q.handoff_state = s->d_state;
        q.handoff_poll_ticks = plan.handoff_poll_ticks; q.handoff_pixels = plan.handoff_pixels;
    }
    if (part.clear_before) HIPCHK(hipMemsetAsync(s->d_tile_cost, 0, plan.ranked_tiles * sizeof(unsigned int), stream));
    if (part.ranked_on != RANK_NONE) RT_TRY(rank_part(s, plan, part, q, stream));
    if (part.clear_after) HIPCHK(hipMemsetAsync(s->d_tile_cost, 0, plan.ranked_tiles * sizeof(unsigned int), stream));   // from here on: measured rays
#ifdef RT_DIAG
    if (last) {   // wave-end histograms of the frame's last launch only (rt_debug_wave_ends)
        HIPCHK(hipMemsetAsync(s->d_ray_counter + RT_DIAG_T0_SLOT, 0xFF, 8, stream));
        HIPCHK(hipMemsetAsync(s->d_ray_counter + RT_DIAG_HIST_SLOT, 0, (size_t)(2 * RT_DIAG_BINS + 7 + 2 * RT_DIAG_MAX_WAVES) * 8, stream));
    }
#endif
    HIPCHK(hipMemsetAsync(s->d_work_counter, 0, RT_WORK_COUNTER_BYTES, stream));
    if (plan.tail_ordered && part.tail) HIPCHK(hipMemsetAsync(s->d_handoff_scratch, 0, RT_HANDOFF_BUCKETS * sizeof(unsigned int), stream));
    const int pi = k & 3;
    if (part.tiers) {
        HIPCHK(hipEventRecord(s->ev_fork[pi], stream));
        HIPCHK(hipStreamWaitEvent(s->tier_stream, s->ev_fork[pi], 0));
        HIPCHK(launch_tier(s, q, dim3(plan.tier_grid), tier_lds, s->tier_stream));
        HIPCHK(hipEventRecord(s->ev_join[pi], s->tier_stream));
    }
    HIPCHK(launch_render(plan.kernel, plan.ml.lds_mode, s, q, dim3(part.grid), plan.ml.block, plan.ml.lds_bytes, stream));
    if (part.tail) {
        // the tail: the pixels the main kernel handed off, one per wave, on whatever the tier kernel -- which may still be
        // running on its own stream: other pixels, other queue head -- leaves free of the machine
        rt_frame_params t = q;
        t.tail_mode = 1;
        if (plan.tail_ordered) {
            // ... served most remaining work first: the tail's waves pull from a copy of the queue ordered on the device
            // (rt_handoff_order.h), like every other queue of the frame.
            rt_handoff_order_params hp;
            memset(&hp, 0, sizeof(hp));
            hp.queue = q.handoff_queue; hp.ordered = s->d_handoff_ordered; hp.state = q.handoff_state;
            hp.pushed = q.work_counter + RT_WC_PUSHED; hp.scratch = s->d_handoff_scratch;
            hp.cap = q.handoff_cap; hp.min_items = plan.order_min; hp.max_items = plan.order_max;
            hp.cost_begin = part.cost_begin; hp.sample_end = q.sample_end;
            HIPCHK(rt_launch_handoff_order(hp, stream));
            t.handoff_queue = s->d_handoff_ordered;
        }
        HIPCHK(launch_tier(s, t, dim3(plan.tail_grid), tier_lds, stream));
    }
    if (part.tiers) HIPCHK(hipStreamWaitEvent(stream, s->ev_join[pi], 0));
    return RT_OK;
}

static rt_status render_impl(rt_scene* s, const rt_frame_desc* f, float* fb, int fb_on_device, void* stream_v, int blocking, rt_stats* stats,
                             rt_progressive* win, int32_t win_begin, int32_t win_end) {
    if (!s || !f || !fb) return invalid("null argument");
    RT_TRY(use_device(s->device));
    // ---- check.  A progressive window averages over the samples rendered so far: win_end, which rt_render_window has checked,
    // stands for f->ns
    frame_geometry g;
    RT_TRY(check_frame(nullptr, f, !win, RENDER_FRAME_TEXTS, g));
    const int frame_ns = win ? win_end : f->ns;
    if (s->frame_pending) RT_TRY(rt_frame_finish(s, nullptr));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);

    rt_stats out;
    memset(&out, 0, sizeof(out));
    out.local_rows = g.local_rows;
    out.samples = (uint64_t)g.local_rows * f->nx * (uint64_t)(win ? win_end - win_begin : f->ns);
    if (g.local_rows == 0) { s->pending_stats = out; if (stats) *stats = out; return RT_OK; }

    // ---- fill
    rt_frame_params fp;
    fill_frame_params(s, f, g, frame_ns, fp);
    const size_t floats = g.n_pixels * 3;
    RT_TRY(device_fb(s, fb, fb_on_device, floats, &fp.fb));
    fp.store_parked = win ? 1 : 0;

    // ---- plan (rt_frame_plan.h): every decision of the frame, made before anything is enqueued
    rt_scene::cost_map_state& cm = s->cost_map;
    const cost_map_view view = {cm.valid, cm.total > 0, cm.key, cm.scene_epoch, cm.opt_epoch, s->scene_epoch, g_opt_epoch};
    frame_plan plan;
    const char* why = nullptr;
    const plan_facts facts = plan_facts_of(s);
    if (plan_frame(facts, g_opt, *f, g, {win != nullptr, win_begin, win_end}, view, plan, why) != RT_OK) return invalid(why);
    if (!plan.ranked) plan.ranked_parts = s->plan.ranked_parts;
    s->plan = plan;
    fp.shade_threshold = plan.ml.shade_threshold; fp.newpath_threshold = plan.ml.newpath_threshold;
    fp.tier_lds_scene = plan.room.lds_scene;
    stats_of_launch(facts, plan.ml, out);
    out.workgroups = (int)plan.parts[plan.n_parts - 1].grid;

    HIPCHK(hipEventRecord(s->ev_start, stream));
    HIPCHK(hipMemsetAsync(s->d_ray_counter, 0, 256, stream));
    // ---- grow the buffers the plan names
    if (plan.ranked) {
        HIPCHK(s->d_tile_cost.grow(plan.ranked_tiles));
        HIPCHK(s->d_tile_order.grow(plan.ranked_tiles));
        HIPCHK(s->d_state.grow(plan.ranked_pixels));
        HIPCHK(s->d_heavy_list.grow(RT_HEAVY_CAP));
        HIPCHK(s->d_heavy_pixels.grow(RT_HEAVY_CAP));
        HIPCHK(s->d_rank.grow(1));
        RT_TRY(cm.grow(plan.cost_map_pixels));
        HIPCHK(s->d_handoff.grow(plan.handoff_capacity));
        if (plan.tail_ordered) {
            HIPCHK(s->d_handoff_ordered.grow(plan.handoff_ordered_capacity));
            HIPCHK(s->d_handoff_scratch.grow(plan.handoff_scratch_words));
        }
        cm.last_key = plan.key; cm.have_last_key = true;
        if (plan.cost_out) { cm.valid = false; cm.key = plan.key; cm.scene_epoch = s->scene_epoch; cm.opt_epoch = g_opt_epoch; }
    }
    // ---- enqueue the parts
    for (int k = 0; k < plan.n_parts; ++k) RT_TRY(launch_part(s, plan, k, fp, win ? win->d_state : s->d_state, stream));
    // ---- the finishing pass (rt_kernel_finish.hip): the main and tier kernels have left every local pixel's colour sum in the
    // frame, each written once by the last part's main, tier or tail launch, all of which the stream has joined; kernel 0 has
    // stored finished pixels.  Inside ev_start .. ev_stop: it is part of the frame's time.
    if (plan.kernel != RT_KERNEL_PIXEL) HIPCHK(rt_launch_finish(fp.fb, floats, frame_ns, f->gamma, stream));
    // ---- finish
    HIPCHK(hipEventRecord(s->ev_stop, stream));
    s->frame_pending = true;
    s->cost_map.pending = plan.cost_out;   // only a frame that was enqueued whole makes its map count (rt_frame_finish)
    s->pending_stream = stream;
    s->pending_stats = out;
    if (!fb_on_device) {
        HIPCHK(hipMemcpyAsync(fb, s->d_fb, floats * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        blocking = 1;
    }
    if (blocking) return rt_frame_finish(s, stats);
    if (stats) *stats = out;
    return RT_OK;
}

// ---- rt_render_adaptive (include/rt_abi.h).  Passes [0, min/2) and [min/2, min) over every pixel, then [c_k, c_k+1)
// over the pixels still active.  The render passes only park pixels (d_adapt_state); the decision kernel (rt_kernel_adaptive.hip)
// writes fb and the sample-count map and compacts the active pixels into the next pass's list (main kernel) and queue (tier kernel).
rt_status rt_render_adaptive(rt_scene* s, const rt_frame_desc* f, const rt_adaptive_desc* a, float* fb, int fb_on_device, int32_t* spp_out,
                             void* stream_v, rt_stats* stats) {
    // argument checks: no HIP call before they pass
    if (!s) return invalid("rt_render_adaptive: null scene");
    if (!f) return invalid("rt_render_adaptive: null frame description");
    if (!a) return invalid("rt_render_adaptive: null adaptive description");
    if (!fb) return invalid("rt_render_adaptive: null fb");
    if (a->min_spp < 2 || (a->min_spp & 1)) return invalid("rt_render_adaptive: min_spp must be even and >= 2");
    int levels = -1;   // K
    for (int k = 0; k <= 16; ++k)
        if ((long long)a->min_spp << k == (long long)a->max_spp) { levels = k; break; }
    if (levels < 0) return invalid("rt_render_adaptive: max_spp must be min_spp * 2^K with 0 <= K <= 16");
    if (!std::isfinite(a->threshold)) return invalid("rt_render_adaptive: threshold is not finite");
    if (!std::isfinite(a->floor) || a->floor < 0.0f) return invalid("rt_render_adaptive: floor must be finite and >= 0");
    frame_geometry g;
    RT_TRY(check_frame("rt_render_adaptive", f, false, {"bad frame size", "bad frame size", "bad row partition", "frame too large"}, g));

    RT_TRY(use_device(s->device));
    if (s->frame_pending) RT_TRY(rt_frame_finish(s, nullptr));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const plan_facts facts = plan_facts_of(s);
    const int min_spp = a->min_spp, max_spp = a->max_spp;
    const size_t n_pixels = g.n_pixels;
    s->adapt_log.clear(); s->adapt_ms.clear();

    rt_stats out;
    memset(&out, 0, sizeof(out));
    out.local_rows = g.local_rows;
    if (n_pixels == 0) { s->pending_stats = out; if (stats) *stats = out; return RT_OK; }

    // ---- buffers: cached in the scene, grown when a frame needs more
    const size_t floats = n_pixels * 3;
    HIPCHK(s->d_adapt_state.grow(n_pixels));      // (rt_render_variance shares the parked pixels and the 4-byte-per-pixel map)
    HIPCHK(s->d_adapt_spp.grow(n_pixels));
    HIPCHK(s->d_adapt_half.grow(n_pixels * 3));
    HIPCHK(s->d_adapt_list[0].grow(n_pixels));
    HIPCHK(s->d_adapt_list[1].grow(n_pixels));
    HIPCHK(s->d_adapt_queue.grow(n_pixels));
    HIPCHK(s->d_adapt_count.grow(16));
    HIPCHK(s->d_adapt_rank.grow(1));
    while (s->adapt_events.size() < 2u * 18u) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        s->adapt_events.push_back(e);
    }
    float* d_fb = nullptr;
    RT_TRY(device_fb(s, fb, fb_on_device, floats, &d_fb));
    int32_t* d_spp = fb_on_device ? spp_out : (spp_out ? s->d_adapt_spp : nullptr);

    // ---- the main kernel's frame parameters (as rt_render_window's, without store_parked: a pass only parks)
    rt_frame_params fp;
    fill_frame_params(s, f, g, max_spp, fp);
    fp.fb = d_fb;
    fp.state_out = s->d_adapt_state;
    const uint32_t all_items = g.work_items;

    // ---- the tier route: the tier kernel's tail mode alone on the machine, one pixel per wave, where the scene has tier data
    // (at most 4096 leaves and 2 media) and its image fits a CU; which passes take it: adaptive_use_tier (rt_frame_plan.h)
    const tier_room room = plan_tier_room(facts, facts.lds_per_cu - 2048);

    int pass_index = 0;
    // one render pass: samples [b, e) of `active` pixels -- every local pixel (list null), or the list / queue the last decision wrote
    auto render_pass = [&](int32_t b, int32_t e, const uint32_t* list, uint32_t active) -> rt_status {
        rt_frame_params q = fp;
        q.sample_begin = b; q.sample_end = e;
        q.state_in = b > 0 ? s->d_adapt_state : nullptr;
        const bool tier = list && adaptive_use_tier(facts, room, g_opt, active);
        hipEvent_t* ev = s->adapt_events.data() + 2 * pass_index;
        HIPCHK(hipEventRecord(ev[0], stream));
        if (tier) {
            // the tail queue (n << 32 | pixel) with the adaptive state as both hand-off state and park target: samples [n, e)
            memset(s->adapt_wc_host, 0, sizeof(s->adapt_wc_host));
            s->adapt_wc_host[RT_WC_PUSHED] = active;   // (the queue head RT_WC_TAIL_HEAD starts at 0)
            HIPCHK(hipMemcpyAsync(s->d_work_counter, s->adapt_wc_host, RT_WORK_COUNTER_BYTES, hipMemcpyHostToDevice, stream));
            q.tail_mode = 1; q.handoff_queue = s->d_adapt_queue; q.handoff_cap = (uint32_t)n_pixels; q.handoff_state = s->d_adapt_state;
            q.tier_lds_scene = room.lds_scene;
            q.work_items = 0;
            const unsigned want = (active + (unsigned)(RT_TIER_THREADS / 64) - 1u) / (unsigned)(RT_TIER_THREADS / 64);
            HIPCHK(launch_tier(s, q, dim3(want < room.tail_grid ? want : room.tail_grid), room.lds, stream));
        } else {
            main_launch ml;
            q.work_items = list ? active : all_items;
            RT_TRY(main_launch_of(facts, RT_KERNEL_STAGED, list ? (size_t)active : n_pixels, q, ml));
            if (pass_index == 0) stats_of_launch(facts, ml, out);
            dim3 grid = ml.grid;
            if (list) {
                // the pixel list is tier 3 of a heavy list (rt_kernel_staged.h stage E): ordinary lanes take its entries first, and
                // with no tiles behind it (work_items 0) a lane that finds it empty is done.  The whole resident grid is launched: the
                // pixels spread over every CU, and waves with few live lanes advance their rays faster
                memset(&s->adapt_rank_host, 0, sizeof(s->adapt_rank_host));
                s->adapt_rank_host.heavy_items = active; s->adapt_rank_host.heavy_threshold = 0xFFFFFFFFu;
                s->adapt_rank_host.sparse_stride = 1; s->adapt_rank_host.semi_stride = 1;
                HIPCHK(hipMemcpyAsync(s->d_adapt_rank, &s->adapt_rank_host, sizeof(rt_rank_info), hipMemcpyHostToDevice, stream));
                q.heavy_pixels = list; q.rank = s->d_adapt_rank; q.work_items = 0;
                grid = dim3((unsigned)(facts.num_cu * ml.per_cu_resident));
            }
            HIPCHK(hipMemsetAsync(s->d_work_counter, 0, RT_WORK_COUNTER_BYTES, stream));
            HIPCHK(launch_render(RT_KERNEL_STAGED, ml.lds_mode, s, q, grid, ml.block, ml.lds_bytes, stream));
        }
        HIPCHK(hipEventRecord(ev[1], stream));
        s->adapt_log.push_back(tier ? 1 : 0); s->adapt_log.push_back((long long)active); s->adapt_log.push_back(b); s->adapt_log.push_back(e);
        out.samples += (uint64_t)active * (uint64_t)(e - b);
        ++pass_index;
        return RT_OK;
    };
    // the decision kernel over the pixels of the pass that just ended (list null: every local pixel)
    auto decide = [&](int mode, int32_t n, const uint32_t* list, uint32_t count, uint32_t* list_out) -> rt_status {
        rt_adaptive_params p;
        memset(&p, 0, sizeof(p));
        p.state = s->d_adapt_state; p.half = s->d_adapt_half; p.list_in = list; p.n_in = count;
        p.list_out = list_out; p.queue_out = s->d_adapt_queue; p.count_out = s->d_adapt_count;
        p.fb = d_fb; p.spp = d_spp; p.n = n; p.mode = mode; p.nx = f->nx;
        p.threshold = a->threshold; p.floor = a->floor; p.gamma = f->gamma;
        HIPCHK(rt_launch_adaptive(p, stream));
        return RT_OK;
    };
    HIPCHK(hipMemsetAsync(s->d_ray_counter, 0, 256, stream));
    HIPCHK(hipEventRecord(s->ev_start, stream));
    const uint32_t all = (uint32_t)n_pixels;
    RT_TRY(render_pass(0, min_spp / 2, nullptr, all));
    if (levels > 0) RT_TRY(decide(RT_ADAPTIVE_SNAPSHOT, min_spp / 2, nullptr, all, nullptr));
    RT_TRY(render_pass(min_spp / 2, min_spp, nullptr, all));
    const uint32_t* list = nullptr;    // the pixels of the pass that just ended (null = every local pixel)
    uint32_t active = all;
    int32_t n = min_spp;
    int which = 0;
    while (n < max_spp && active > 0) {
        uint32_t* next = s->d_adapt_list[which];
        HIPCHK(hipMemsetAsync(s->d_adapt_count, 0, sizeof(uint32_t), stream));
        RT_TRY(decide(RT_ADAPTIVE_DECIDE, n, list, active, next));
        HIPCHK(hipMemcpyAsync(&active, s->d_adapt_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        list = next; which ^= 1;
        if (active == 0) break;
        RT_TRY(render_pass(n, 2 * n, list, active));
        n *= 2;
    }
    if (n == max_spp && active > 0) RT_TRY(decide(RT_ADAPTIVE_FINAL, n, list, active, nullptr));
    HIPCHK(hipEventRecord(s->ev_stop, stream));
    if (!fb_on_device) {
        HIPCHK(hipMemcpyAsync(fb, d_fb, floats * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (spp_out) HIPCHK(hipMemcpyAsync(spp_out, d_spp, n_pixels * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    }
    RT_TRY(finish_sync_frame(s, stream, pass_index, out, stats));
    for (int k = 0; k < pass_index; ++k) {
        float pm = 0.f;
        HIPCHK(hipEventElapsedTime(&pm, s->adapt_events[2 * k], s->adapt_events[2 * k + 1]));
        s->adapt_ms.push_back(pm);
    }
    return RT_OK;
}

// ---- rt_render_variance (include/rt_abi.h).  B passes [c_{b-1}, c_b) over every pixel on the main kernel, as
// rt_render_adaptive's first two passes run (they only park pixels, d_adapt_state in and out); after each the batch-means kernel
// (rt_kernel_variance.hip) updates 24 bytes per pixel, and after the last it writes fb and the variance.  One enqueue, one wait.
rt_status rt_render_variance(rt_scene* s, const rt_frame_desc* f, const rt_variance_desc* v, float* fb, int fb_on_device, float* variance_out,
                             void* stream_v, rt_stats* stats) {
    // argument checks: no HIP call before they pass
    if (!s) return invalid("rt_render_variance: null scene");
    if (!f) return invalid("rt_render_variance: null frame description");
    if (!v) return invalid("rt_render_variance: null variance description");
    if (!fb) return invalid("rt_render_variance: null fb");
    if (!variance_out) return invalid("rt_render_variance: null variance_out");
    if (v->batches < 2 || v->batches > 64) return invalid("rt_render_variance: batches must be in 2..64");
    if (f->ns <= 0 || f->ns % v->batches != 0) return invalid("rt_render_variance: ns must be a positive multiple of batches");
    frame_geometry g;
    RT_TRY(check_frame("rt_render_variance", f, false, {"bad frame size", "bad frame size", "bad row partition", "bad frame size (too many 8x8 tiles)"}, g));

    RT_TRY(use_device(s->device));
    if (s->frame_pending) RT_TRY(rt_frame_finish(s, nullptr));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const int B = v->batches, per = f->ns / B;
    s->adapt_log.clear(); s->adapt_ms.clear();   // (rt_debug_adaptive_passes reports the last adaptive frame: this is none)
    const size_t n_pixels = g.n_pixels;

    rt_stats out;
    memset(&out, 0, sizeof(out));
    out.local_rows = g.local_rows;
    out.samples = (uint64_t)n_pixels * (uint64_t)f->ns;
    if (n_pixels == 0) { s->pending_stats = out; if (stats) *stats = out; return RT_OK; }

    // ---- buffers: the adaptive frame's parked pixels and 4-byte-per-pixel map, the accumulators (T_{b-1}, A, Q: three doubles
    // per pixel), a host fb's device image
    const size_t floats = n_pixels * 3;
    HIPCHK(s->d_adapt_state.grow(n_pixels));
    HIPCHK(s->d_adapt_spp.grow(n_pixels));
    HIPCHK(s->d_var_acc.grow(n_pixels * 3));
    float* d_fb = nullptr;
    RT_TRY(device_fb(s, fb, fb_on_device, floats, &d_fb));
    float* d_var = fb_on_device ? variance_out : reinterpret_cast<float*>(s->d_adapt_spp.get());

    // ---- the main kernel's frame parameters (rt_render_adaptive's: a pass only parks)
    rt_frame_params fp;
    fill_frame_params(s, f, g, f->ns, fp);
    fp.fb = d_fb;
    fp.state_out = s->d_adapt_state;
    main_launch ml;
    const plan_facts facts = plan_facts_of(s);
    RT_TRY(main_launch_of(facts, RT_KERNEL_STAGED, n_pixels, fp, ml));
    stats_of_launch(facts, ml, out);

    rt_variance_params vp;
    memset(&vp, 0, sizeof(vp));
    vp.state = s->d_adapt_state; vp.acc = s->d_var_acc; vp.fb = d_fb; vp.variance = d_var;
    vp.n_pixels = (uint32_t)n_pixels; vp.per = per; vp.batches = B; vp.nx = f->nx; vp.gamma = f->gamma;

    HIPCHK(hipMemsetAsync(s->d_ray_counter, 0, 256, stream));
    HIPCHK(hipEventRecord(s->ev_start, stream));
    for (int b = 1; b <= B; ++b) {
        rt_frame_params q = fp;
        q.sample_begin = (b - 1) * per; q.sample_end = b * per;
        q.state_in = b > 1 ? s->d_adapt_state : nullptr;
        HIPCHK(hipMemsetAsync(s->d_work_counter, 0, RT_WORK_COUNTER_BYTES, stream));
        HIPCHK(launch_render(RT_KERNEL_STAGED, ml.lds_mode, s, q, ml.grid, ml.block, ml.lds_bytes, stream));
        vp.c = b * per; vp.first = b == 1; vp.last = b == B;
        HIPCHK(rt_launch_variance(vp, stream));
    }
    HIPCHK(hipEventRecord(s->ev_stop, stream));
    if (!fb_on_device) {
        HIPCHK(hipMemcpyAsync(fb, d_fb, floats * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(variance_out, d_var, n_pixels * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    return finish_sync_frame(s, stream, B, out, stats);
}

}  // extern "C"
