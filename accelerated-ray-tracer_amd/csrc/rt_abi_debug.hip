// rt_abi_debug.hip -- the rt_debug_* entries of include/rt_abi.h: read-backs of what a scene's last frame left (diagnostics,
// every build) and the test seams, which run one launch of a kernel family once, on caller-supplied host data, on the null stream
// and synchronously.  Every seam is its argument checks -- all of them before any HIP call --, its parameter block and its rows
// of a seam_arrays.  No kernel here; the host internals are rt_host.h's.
#include <algorithm>
#include <cmath>

#include "rt_host.h"
#include "rt_handoff_order.h"

using namespace rt_host;

namespace {
// The device arrays of one seam call.  An input row copies `bytes` from the host into fresh device memory; an output row gets
// fresh device memory filled with a tell-tale byte, which comes back to the host after the launch (host null: nowhere); either
// stores the device pointer into the parameter block.  run() takes the launch's status, waits and makes the copies back.  (A HIP
// error is reported with the line and expression here, not the seam's.)
class seam_arrays {
    call_memory mem;
    struct copy_back { void* host; const void* dev; size_t bytes; };
    std::vector<copy_back> backs;
public:
    template <class P> rt_status in(P* slot, const void* host, size_t bytes) {
        void* d = nullptr;
        HIPCHK(mem.get(&d, bytes));
        if (bytes) HIPCHK(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
        *slot = static_cast<P>(d);
        return RT_OK;
    }
    // an input the kernel also writes: `host` is read before and written after the launch
    template <class P> rt_status inout(P* slot, void* host, size_t bytes) {
        RT_TRY(in(slot, host, bytes));
        backs.push_back({host, *slot, bytes});
        return RT_OK;
    }
    template <class P> rt_status out(P* slot, void* host, size_t bytes, int fill) {
        void* d = nullptr;
        HIPCHK(mem.get(&d, bytes));
        if (bytes) HIPCHK(hipMemset(d, fill, bytes));
        *slot = static_cast<P>(d);
        backs.push_back({host, d, bytes});
        return RT_OK;
    }
    rt_status run(hipError_t launched) {
        HIPCHK(launched);
        HIPCHK(hipDeviceSynchronize());
        for (const copy_back& b : backs)
            if (b.host && b.bytes) HIPCHK(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
        return RT_OK;
    }
};
// The rt_pixel_state::cost column of the ranking seams: `n` parked pixels (and `spare` more) whose costs are cost[0 .. n), every
// other field zero; and the costs back out of them.
std::vector<rt_pixel_state> parked(const uint32_t* cost, size_t n, size_t spare = 0) {
    std::vector<rt_pixel_state> state(n + spare);                      // (value-initialised)
    for (size_t i = 0; i < n; ++i) state[i].cost = cost[i];
    return state;
}
void costs_of(const std::vector<rt_pixel_state>& state, uint32_t* cost_out) {
    for (size_t i = 0; i < state.size(); ++i) cost_out[i] = state[i].cost;
}
}  // namespace

extern "C" {

rt_status rt_debug_scene_quads(const rt_scene* s, rt_quad* quads_out, int32_t quad_cap, rt_box* boxes_out, int32_t box_cap) {
    if (!s) return invalid("rt_debug_scene_quads: null scene");
    if ((quads_out && quad_cap < s->n_quads) || (boxes_out && box_cap < s->n_boxes)) return invalid("rt_debug_scene_quads: a cap is below the scene's count");
    RT_TRY(use_device(s->device));
    if (quads_out && s->n_quads) HIPCHK(hipMemcpy(quads_out, s->dev.quads, (size_t)s->n_quads * sizeof(rt_quad), hipMemcpyDeviceToHost));
    if (boxes_out && s->n_boxes) HIPCHK(hipMemcpy(boxes_out, s->dev.boxes, (size_t)s->n_boxes * sizeof(rt_box), hipMemcpyDeviceToHost));
    return RT_OK;
}

rt_status rt_debug_scene_boxes(const rt_scene* s, int32_t which, void* out, size_t cap, size_t* n) {
    if (!s || !n || which < 0 || which > 5) return invalid("rt_debug_scene_boxes: bad argument");
    const void* src = nullptr;
    size_t bytes = 0;
    if (which == 0) { src = s->dev.nodes_ref; bytes = (size_t)s->dev.n_nodes_ref * sizeof(rt_node); }
    else if (which == 1) { src = s->dev.nodes; bytes = (size_t)s->dev.n_nodes * sizeof(rt_node); }
    else if (which == 2 || which == 3) { src = which == 2 ? s->dev.leaf_lo : s->dev.leaf_hi; bytes = src ? (size_t)s->dev.n_slots * 64 * sizeof(float4) : 0; }
    else if (which == 4) { src = s->dev.slot_ranges; bytes = src ? (size_t)s->dev.n_slots * 32 : 0; }
    *n = which == 5 ? 12 : bytes;
    const size_t take = std::min(*n, cap);
    if (!out || take == 0) return RT_OK;
    if (which == 5) { memcpy(out, s->dev.bound, take); return RT_OK; }
    RT_TRY(use_device(s->device));
    HIPCHK(hipMemcpy(out, src, take, hipMemcpyDeviceToHost));
    return RT_OK;
}

// Tail hand-off of the last frame (diagnostics, every build): [0] pixels the main kernel handed to the tail launches, summed over
// the frame's parts, [1] the samples those pixels still had to go.
rt_status rt_debug_handoff(rt_scene* s, unsigned long long* out2) {
    if (!s || !out2) return invalid("null argument");
    RT_TRY(use_device(s->device));
    HIPCHK(hipMemcpy(out2, s->d_ray_counter + 28, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RT_OK;
}

// The hand-off queue of the last frame's last part, in push order (diagnostics, every build; tools/tail_order_stats.py): up to `cap`
// entries (next sample << 32 | pixel), entry for entry the parked cost handoff_state[pixel].cost, and the queue as the tail launch
// was given it (`served`: ordered, copied through, or -- handoff_order = 0 -- the queue itself).  info4: [0] entries the queue
// holds, [1] 1 = the ordering kernels ran, [2] and [3] the counts between which they order (rt_handoff_order.h).  A pending
// frame must have been closed.
rt_status rt_debug_handoff_queue(rt_scene* s, unsigned long long* entries, uint32_t* costs, unsigned long long* served, int64_t cap, int64_t* info4) {
    if (!s || !info4 || cap < 0 || (cap > 0 && (!entries || !costs || !served))) return invalid("rt_debug_handoff_queue: bad argument");
    if (s->frame_pending) return invalid("rt_debug_handoff_queue: a frame is pending (rt_frame_finish first)");
    info4[0] = 0; info4[1] = s->plan.tail_ordered ? 1 : 0; info4[2] = s->plan.order_min; info4[3] = s->plan.order_max;
    int64_t* const count_out = info4;
    if (!s->d_handoff || !s->d_state || !s->plan.ranked) return RT_OK;
    RT_TRY(use_device(s->device));
    unsigned int pushed = 0;
    HIPCHK(hipMemcpy(&pushed, s->d_work_counter + RT_WC_PUSHED, sizeof(pushed), hipMemcpyDeviceToHost));
    const size_t count = pushed < s->d_handoff.capacity() ? pushed : s->d_handoff.capacity();
    *count_out = (int64_t)count;
    const size_t n = count < (size_t)cap ? count : (size_t)cap;
    if (n == 0) return RT_OK;
    HIPCHK(hipMemcpy(entries, s->d_handoff, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(served, s->plan.tail_ordered ? s->d_handoff_ordered.get() : s->d_handoff.get(), n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::vector<rt_pixel_state> h_state(s->d_state.capacity());
    HIPCHK(hipMemcpy(h_state.data(), s->d_state, h_state.size() * sizeof(rt_pixel_state), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        const uint32_t pix = (uint32_t)entries[i];
        costs[i] = pix < h_state.size() ? h_state[pix].cost : 0u;
    }
    return RT_OK;
}

// Test seam of the queue ordering (rt_handoff_order.h; tests/test_handoff_order.py): the launch rt_render makes between the main
// kernel and the tail launch, once, on n caller-supplied entries (next sample << 32 | pixel, every pixel below n) whose parked
// costs are costs[pixel], for a tail launch of tail_waves waves and a part rendering [sample_begin, sample_end).  Null stream, synchronous.
// The queue holds exactly n entries and the push counter stands ORDER_SEAM_SLACK beyond, as after a main kernel whose lanes found
// the queue full; both device buffers have that many spare slots behind them, and *overrun_out = how many of the ordered
// buffer's were written (0 unless the count was read unclipped).
enum { ORDER_SEAM_SLACK = 3 };
rt_status rt_debug_order_handoff(const unsigned long long* entries, const uint32_t* costs, int64_t n, int32_t sample_begin, int32_t sample_end,
                                 int32_t tail_waves, unsigned long long* out, uint32_t* overrun_out) {
    if (!overrun_out) return invalid("rt_debug_order_handoff: null argument");
    if (n < 0 || n > (1ll << 24) || (n > 0 && (!entries || !costs || !out))) return invalid("rt_debug_order_handoff: n must be 0 .. 2^24 and the arrays non-null");
    if (sample_begin < 0 || sample_end < sample_begin) return invalid("rt_debug_order_handoff: bad sample range");
    if (tail_waves < 1 || tail_waves > (1 << 20)) return invalid("rt_debug_order_handoff: tail_waves must be 1 .. 2^20");
    for (int64_t i = 0; i < n; ++i)
        if ((int64_t)(uint32_t)entries[i] >= n) return invalid("rt_debug_order_handoff: an entry's pixel is not below n");
    RT_TRY(use_device(g_device));
    rt_handoff_order_params hp;
    memset(&hp, 0, sizeof(hp));
    const size_t most = (size_t)RT_HANDOFF_ORDER_MAX_PER_WAVE * (size_t)tail_waves;
    hp.cap = (uint32_t)n; hp.min_items = (uint32_t)(RT_HANDOFF_ORDER_MIN_PER_WAVE * tail_waves); hp.max_items = (uint32_t)(most < (size_t)n ? most : (size_t)n);
    hp.cost_begin = sample_begin; hp.sample_end = sample_end;
    const size_t slots = (size_t)n + ORDER_SEAM_SLACK;
    std::vector<unsigned long long> queue(slots, 0ull), ordered(slots);          // spare slots of the queue: sample 0 of pixel 0
    std::copy(entries, entries + n, queue.begin());
    const std::vector<rt_pixel_state> state = parked(costs, (size_t)n, 1);
    const unsigned int pushed = (unsigned int)slots;
    seam_arrays arrays;
    RT_TRY(arrays.in(&hp.queue, queue.data(), slots * sizeof(unsigned long long)));
    RT_TRY(arrays.out(&hp.ordered, ordered.data(), slots * sizeof(unsigned long long), 0xFF));
    RT_TRY(arrays.in(&hp.state, state.data(), state.size() * sizeof(rt_pixel_state)));
    RT_TRY(arrays.in(&hp.pushed, &pushed, sizeof(pushed)));
    RT_TRY(arrays.out(&hp.scratch, nullptr, rt_handoff_order_scratch_words(hp.max_items) * sizeof(unsigned int), 0));
    RT_TRY(arrays.run(rt_launch_handoff_order(hp, nullptr)));
    std::copy(ordered.begin(), ordered.begin() + n, out);
    *overrun_out = 0u;
    for (size_t k = (size_t)n; k < slots; ++k) *overrun_out += ordered[k] != ~0ull ? 1u : 0u;
    return RT_OK;
}

// Diagnostic builds (-DRT_DIAG) leave per-stage execution counts behind the ray counter; 16 values.
rt_status rt_debug_counters(rt_scene* s, unsigned long long* out16) {
    if (!s || !out16) return invalid("null argument");
    RT_TRY(use_device(s->device));
    HIPCHK(hipMemcpy(out16, s->d_ray_counter + 1, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RT_OK;
}
// Diagnostic builds: cycles the waves of the frame spent per part of the staged kernel's loop, summed over waves
// ([0] box steps, [1] object tests, [2] stage C, [3] D, [4] E, [6] stage gating, [7] stage F + loop; then, first wave of each
// tier workgroup: [8] resolve + shade in the tier loops, [9] the whole tier loop; shader-clock cycles).
rt_status rt_debug_stage_cycles(rt_scene* s, unsigned long long* out10) {
    if (!s || !out10) return invalid("null argument");
    RT_TRY(use_device(s->device));
    HIPCHK(hipMemcpy(out10, s->d_ray_counter + 17, 10 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RT_OK;
}
// Diagnostic builds: when the waves of the LAST launch ended, as two histograms of RT_DIAG_BINS bins of 1 ms after the first
// wave's start (ordinary waves, then waves that started in sparse / tier mode).
rt_status rt_debug_wave_ends(rt_scene* s, unsigned long long* out, int n) {
    if (!s || !out || n < 0 || n > 2 * RT_DIAG_BINS) return invalid("bad argument");
    RT_TRY(use_device(s->device));
    HIPCHK(hipMemcpy(out, s->d_ray_counter + RT_DIAG_HIST_SLOT, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RT_OK;
}
// ... and per wave of the last launch, two words about the lane that ran out of work last: (done_us << 32 | fetch_us of its last
// pixel), (source queue << 60 | started sparse << 59 | local pixel id)
rt_status rt_debug_wave_last(rt_scene* s, unsigned long long* out, int n_waves) {
    if (!s || !out || n_waves < 0 || n_waves > RT_DIAG_MAX_WAVES) return invalid("bad argument");
    RT_TRY(use_device(s->device));
    HIPCHK(hipMemcpy(out, s->d_ray_counter + RT_DIAG_WAVE_SLOT, (size_t)2 * n_waves * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- test seams of the ranking and the cost prior (rt_rank.hip; tests/test_rank.py): the launches rt_render makes, once, on
// caller-supplied host data.  Null stream, synchronous; every check runs before any HIP call.
enum { RANK_PARAM_WORDS = 20, RANK_INFO_WORDS = 13 };
static_assert(sizeof(rt_rank_info) == RANK_INFO_WORDS * 4, "rt_debug_rank / rt_debug_rank_info copy rt_rank_info as 13 words");

rt_status rt_debug_rank(const uint32_t* cost, const uint32_t* tile_cost, uint64_t rays, const uint32_t* params, uint32_t* tile_order,
                        uint32_t* cost_out, uint32_t* heavy_pixels, uint32_t* info13) {
    if (!cost || !tile_cost || !params || !tile_order || !cost_out || !heavy_pixels || !info13) return invalid("rt_debug_rank: null argument");
    rt_rank_params rp;
    memset(&rp, 0, sizeof(rp));
    const int32_t* ip = reinterpret_cast<const int32_t*>(params);
    rp.n_pixels = params[0]; rp.n_tiles = params[1]; rp.heavy_cap = params[2];
    rp.max_grid = params[3]; rp.waves_per_wg = params[4]; rp.normal_need = params[5];
    rp.sparse_stride = ip[6]; rp.semi_stride = ip[7]; rp.sparse_percent = ip[8]; rp.sparse_work_percent = ip[9];
    rp.tier_possible = ip[10]; rp.tier1_pixels = ip[11]; rp.tier1_depth = ip[12]; rp.tier_wgs_cap = ip[13];
    rp.tier_waves_per_main_wg = ip[14]; rp.nx = ip[15]; rp.smooth_percent = ip[16];
    memcpy(&rp.heavy_factor, params + 17, 4); memcpy(&rp.sparse_factor, params + 18, 4); memcpy(&rp.tier1_factor, params + 19, 4);
    if (rp.n_pixels < 1u || rp.n_pixels >= (1u << 31)) return invalid("rt_debug_rank: n_pixels must be 1 .. 2^31 - 1");
    if (rp.n_tiles < 1u || rp.n_tiles > rp.n_pixels) return invalid("rt_debug_rank: n_tiles must be 1 .. n_pixels");
    if (rp.heavy_cap < 1u || rp.heavy_cap > (1u << 24)) return invalid("rt_debug_rank: heavy_cap must be 1 .. 2^24");
    if (rp.max_grid > (1u << 20) || rp.normal_need > (1u << 20)) return invalid("rt_debug_rank: max_grid and normal_need must be at most 2^20");
    if (rp.waves_per_wg < 1u || rp.waves_per_wg > 16u) return invalid("rt_debug_rank: waves_per_wg must be 1 .. 16");
    if (rp.sparse_stride < 0 || rp.sparse_stride > 64 || rp.semi_stride < 0 || rp.semi_stride > 64) return invalid("rt_debug_rank: sparse_stride and semi_stride must be 0 .. 64");
    if (rp.sparse_percent < 0 || rp.sparse_percent > 100 || rp.sparse_work_percent < 0 || rp.sparse_work_percent > 100 || rp.smooth_percent < 0 || rp.smooth_percent > 100)
        return invalid("rt_debug_rank: sparse_percent, sparse_work_percent and smooth_percent must be 0 .. 100");
    if (rp.tier1_pixels < 0 || rp.tier1_depth < 0 || rp.tier1_depth > 65536 || rp.tier_wgs_cap < 0 || rp.tier_waves_per_main_wg < 0)
        return invalid("rt_debug_rank: tier1_pixels, tier1_depth (at most 65536), tier_wgs_cap and tier_waves_per_main_wg must not be negative");
    if (rp.nx < 1 || (uint32_t)rp.nx > rp.n_pixels) return invalid("rt_debug_rank: nx must be 1 .. n_pixels");
    float top = 0.f;
    for (const float fac : {rp.heavy_factor, rp.sparse_factor, rp.tier1_factor}) {
        if (!(fac >= 0.f) || !(fac <= 1000.f)) return invalid("rt_debug_rank: the three factors must be 0 .. 1000");
        top = fac > top ? fac : top;
    }
    if (!((double)rays / (double)rp.n_pixels * (double)top + 1.0 < 4294967296.0)) return invalid("rt_debug_rank: rays / n_pixels x the largest factor must stay below 2^32");
    RT_TRY(use_device(g_device));
    std::vector<rt_pixel_state> state = parked(cost, rp.n_pixels);     // (every field but the cost is zero)
    const unsigned long long h_rays = rays;
    const size_t tiles = (size_t)rp.n_tiles * sizeof(unsigned int);
    seam_arrays arrays;   // entries the ranking does not write stay 0xFFFFFFFF
    RT_TRY(arrays.inout(&rp.state, state.data(), state.size() * sizeof(rt_pixel_state)));
    RT_TRY(arrays.in(&rp.tile_cost, tile_cost, tiles));
    RT_TRY(arrays.out(&rp.tile_order, tile_order, tiles, 0xFF));
    RT_TRY(arrays.in(&rp.ray_counter, &h_rays, sizeof(h_rays)));
    RT_TRY(arrays.out(&rp.heavy_list, nullptr, (size_t)rp.heavy_cap * sizeof(unsigned long long), 0xFF));
    RT_TRY(arrays.out(&rp.heavy_pixels, heavy_pixels, (size_t)rp.heavy_cap * sizeof(unsigned int), 0xFF));
    RT_TRY(arrays.out(&rp.info, info13, sizeof(rt_rank_info), 0xFF));
    RT_TRY(arrays.run(rt_launch_rank(rp, nullptr)));
    costs_of(state, cost_out);
    return RT_OK;
}

rt_status rt_debug_prior(const uint32_t* cal_cost, int32_t cal_nx, int32_t cal_ny, int32_t nx, int32_t ny, int32_t tile_rows, int32_t tile_first,
                         int32_t tile_stride, uint32_t* cost_out, uint32_t* tile_cost_out, uint64_t* total_out) {
    if (!cal_cost || !cost_out || !tile_cost_out || !total_out) return invalid("rt_debug_prior: null argument");
    if (cal_nx < 1 || cal_ny < 1 || (long long)cal_nx * cal_ny >= (1ll << 31)) return invalid("rt_debug_prior: bad calibration grid size");
    rt_frame_desc f;
    memset(&f, 0, sizeof(f));
    f.nx = nx; f.ny = ny; f.tile_rows = tile_rows; f.tile_first = tile_first; f.tile_stride = tile_stride;
    frame_geometry g;
    RT_TRY(check_frame("rt_debug_prior", &f, false, STATE_FRAME_TEXTS, g));
    if (g.local_rows == 0) return invalid("rt_debug_prior: the partition has no rows");
    RT_TRY(use_device(g_device));
    rt_prior_params pp;
    memset(&pp, 0, sizeof(pp));
    pp.cal_nx = cal_nx; pp.cal_ny = cal_ny; pp.nx = nx; pp.ny = ny; pp.local_rows = g.local_rows; pp.tiles_x = g.tiles_x;
    pp.tile_rows = tile_rows; pp.tile_first = tile_first; pp.tile_stride = tile_stride;
    const size_t n_tiles = (size_t)g.tiles_x * (size_t)g.tiles_y, n_cal = (size_t)cal_nx * (size_t)cal_ny;
    std::vector<rt_pixel_state> state(g.n_pixels);
    unsigned long long total = 0;
    seam_arrays arrays;
    RT_TRY(arrays.out(&pp.state, state.data(), state.size() * sizeof(rt_pixel_state), 0xFF));   // a pixel the kernel skips shows as 0xFFFFFFFF
    RT_TRY(arrays.out(&pp.tile_cost, tile_cost_out, n_tiles * sizeof(unsigned int), 0));        // (the kernel adds to both, as in rt_render)
    RT_TRY(arrays.out(&pp.total, &total, sizeof(total), 0));
    RT_TRY(arrays.in(&pp.cal_cost, cal_cost, n_cal * sizeof(unsigned int)));
    RT_TRY(arrays.run(rt_launch_prior(pp, nullptr)));
    costs_of(state, cost_out);
    *total_out = total;
    return RT_OK;
}

rt_status rt_debug_box_tests(int32_t n, const float* bmin, const float* bmax, const float* origins, const float* directions,
                             const float* tmin, const float* tmax, const float* bound3, uint8_t* flags) {
    if (!bmin || !bmax || !origins || !directions || !tmin || !tmax || !bound3 || !flags) return invalid("rt_debug_box_tests: null argument");
    if (n < 1 || n > (1 << 24)) return invalid("rt_debug_box_tests: n must be 1 .. 2^24");
    for (int k = 0; k < 3; ++k)
        if (!(bound3[k] >= 0.f) || !std::isfinite(bound3[k])) return invalid("rt_debug_box_tests: bound3 must be finite and not negative");
    RT_TRY(use_device(g_device));
    rt_box_test_params bp;
    memset(&bp, 0, sizeof(bp));
    bp.n = n;
    for (int k = 0; k < 3; ++k) bp.bound[k] = bound3[k];
    const size_t n3 = (size_t)n * 3 * sizeof(float), n1 = (size_t)n * sizeof(float);
    seam_arrays arrays;
    RT_TRY(arrays.in(&bp.bmin, bmin, n3));
    RT_TRY(arrays.in(&bp.bmax, bmax, n3));
    RT_TRY(arrays.in(&bp.origins, origins, n3));
    RT_TRY(arrays.in(&bp.directions, directions, n3));
    RT_TRY(arrays.in(&bp.tmin, tmin, n1));
    RT_TRY(arrays.in(&bp.tmax, tmax, n1));
    RT_TRY(arrays.out(&bp.flags, flags, (size_t)n * 4, 0xFF));   // a case the kernel skipped would show as 255
    return arrays.run(rt_launch_box_tests(bp, nullptr));
}

rt_status rt_debug_arith_tests(int32_t mode, int64_t n, const float* a, const float* b, const float* bound3, uint8_t* path, uint64_t* out3) {
    if (mode < RT_ARITH_UNIFORM || mode > RT_ARITH_LOOSE) return invalid("rt_debug_arith_tests: unknown mode");
    const bool draws = mode == RT_ARITH_UNIFORM || mode == RT_ARITH_SIGNED;
    if (!out3 || (!draws && (!a || !b || !bound3))) return invalid("rt_debug_arith_tests: null argument");
    if (draws && path) return invalid("rt_debug_arith_tests: the draw modes report no path");
    if (draws ? (n < 1 || n > (1ll << 32)) : (n < 1 || n > (1 << 24))) return invalid(draws ? "rt_debug_arith_tests: n must be 1 .. 2^32" : "rt_debug_arith_tests: n must be 1 .. 2^24");
    if (!draws)
        for (int k = 0; k < 3; ++k)
            if (!(bound3[k] >= 0.f) || !std::isfinite(bound3[k])) return invalid("rt_debug_arith_tests: bound3 must be finite and not negative");
    RT_TRY(use_device(g_device));
    rt_arith_test_params ap;
    memset(&ap, 0, sizeof(ap));
    ap.mode = mode; ap.n = n;
    seam_arrays arrays;
    if (!draws) {
        for (int k = 0; k < 3; ++k) ap.bound[k] = bound3[k];
        const size_t n3 = (size_t)n * 3 * sizeof(float);
        RT_TRY(arrays.in(&ap.a, a, n3));
        RT_TRY(arrays.in(&ap.b, b, n3));
        if (path) RT_TRY(arrays.out(&ap.path, path, (size_t)n, 0xFF));   // a case the kernel skipped would show as 255
    }
    unsigned long long counts[3] = {0ull, ~0ull, 0ull};
    RT_TRY(arrays.inout(&ap.out, counts, sizeof(counts)));
    RT_TRY(arrays.run(rt_launch_arith_tests(ap, nullptr)));
    for (int k = 0; k < 3; ++k) out3[k] = counts[k];
    return RT_OK;
}

rt_status rt_debug_math_tests(int32_t form, int32_t fn, uint32_t first, int64_t count, float operand, const float* a, const float* b,
                              const float* c, float* out, uint64_t* digests) {
    if (form != RT_MATH_SWEEP && form != RT_MATH_LIST) return invalid("rt_debug_math_tests: unknown form");
    if (fn < RT_MATH_LOG || fn > RT_MATH_MULADD) return invalid("rt_debug_math_tests: unknown function");
    const bool sweep = form == RT_MATH_SWEEP;
    const bool reads_b = fn == RT_MATH_ATAN2 || fn == RT_MATH_POW || fn == RT_MATH_DIV || fn == RT_MATH_MULADD, reads_c = fn == RT_MATH_MULADD;
    if (sweep) {
        if (reads_b && fn != RT_MATH_POW) return invalid("rt_debug_math_tests: a sweep takes a function of one input, or RT_MATH_POW");
        if (!digests) return invalid("rt_debug_math_tests: null argument");
        if (a || b || c || out) return invalid("rt_debug_math_tests: a sweep reads no array and writes digests only");
        if (count < 1 || count > (1ll << 32) || (int64_t)first + count > (1ll << 32)) return invalid("rt_debug_math_tests: count must be 1 .. 2^32 and first + count at most 2^32");
        if (fn == RT_MATH_POW && (!(operand > 0.f) || !std::isfinite(operand))) return invalid("rt_debug_math_tests: gamma must be finite and positive");
    } else {
        if (!a || !out || (reads_b && !b) || (reads_c && !c)) return invalid("rt_debug_math_tests: null argument");
        if (digests) return invalid("rt_debug_math_tests: a list writes out only");
        if (count < 1 || count > (1 << 24) || first != 0u) return invalid("rt_debug_math_tests: count must be 1 .. 2^24 and first 0");
    }
    RT_TRY(use_device(g_device));
    rt_math_test_params mp;
    memset(&mp, 0, sizeof(mp));
    mp.form = form; mp.fn = fn; mp.first = first; mp.count = count; mp.operand = operand;
    const size_t n_digests = (size_t)((count + (1ll << 20) - 1) >> 20), list_bytes = (size_t)count * sizeof(float);
    seam_arrays arrays;
    if (sweep) {
        RT_TRY(arrays.out(&mp.digests, digests, n_digests * sizeof(unsigned long long), 0));
    } else {
        RT_TRY(arrays.in(&mp.a, a, list_bytes));
        if (reads_b) RT_TRY(arrays.in(&mp.b, b, list_bytes));
        if (reads_c) RT_TRY(arrays.in(&mp.c, c, list_bytes));
        RT_TRY(arrays.out(&mp.out, out, list_bytes, 0xFF));   // an element the kernel skipped would show as a NaN with payload
    }
    return arrays.run(rt_launch_math_tests(mp, nullptr));
}

rt_status rt_debug_cal_cost(rt_scene* s, uint32_t* out, int32_t cap, int32_t* nx, int32_t* ny) {
    if (!s) return invalid("rt_debug_cal_cost: null scene");
    if (!out || !nx || !ny) return invalid("rt_debug_cal_cost: null argument");
    if (cap < 64) return invalid("rt_debug_cal_cost: cap must be at least 64 (the smallest calibration grid is 8 x 8)");
    if (!s->d_cal_cost || s->cal_nx <= 0 || s->cal_ny <= 0) return invalid("rt_debug_cal_cost: the scene kept no calibration costs");
    *nx = s->cal_nx; *ny = s->cal_ny;
    if ((long long)cap < (long long)s->cal_nx * s->cal_ny) return invalid("rt_debug_cal_cost: cap is smaller than the calibration grid (nx and ny are set)");
    RT_TRY(use_device(s->device));
    HIPCHK(hipMemcpy(out, s->d_cal_cost, (size_t)s->cal_nx * s->cal_ny * sizeof(unsigned int), hipMemcpyDeviceToHost));
    return RT_OK;
}

rt_status rt_debug_cost_map(rt_scene* s, uint32_t* out, int64_t cap, int32_t* info4) {
    if (!s) return invalid("rt_debug_cost_map: null scene");
    if (!info4 || (!out && cap != 0)) return invalid("rt_debug_cost_map: null argument");
    RT_TRY(use_device(s->device));
    if (s->frame_pending) RT_TRY(rt_frame_finish(s, nullptr));
    const rt_scene::cost_map_state& cm = s->cost_map;
    const bool have = g_opt.cost_map && cm.valid;
    info4[0] = !have ? 0 : (cm.scene_epoch == s->scene_epoch && cm.opt_epoch == g_opt_epoch ? 1 : 2);
    info4[1] = have ? cm.key.nx : 0; info4[2] = have ? cm.key.local_rows : 0; info4[3] = s->plan.ranked_parts;
    if (!have || !out) return RT_OK;
    const long long n = (long long)cm.key.nx * cm.key.local_rows;
    if ((long long)cap < n) return invalid("rt_debug_cost_map: cap is smaller than the map (info is set)");
    HIPCHK(hipMemcpy(out, cm.d, (size_t)n * sizeof(unsigned int), hipMemcpyDeviceToHost));
    return RT_OK;
}

rt_status rt_debug_set_cost_map(rt_scene* s, const uint32_t* in, int64_t n) {
    if (!s) return invalid("rt_debug_set_cost_map: null scene");
    if (!in) return invalid("rt_debug_set_cost_map: null argument");
    if (!g_opt.cost_map) return invalid("rt_debug_set_cost_map: option cost_map is 0");
    rt_scene::cost_map_state& cm = s->cost_map;
    if (!cm.have_last_key) return invalid("rt_debug_set_cost_map: the scene has rendered no ranked frame");
    if ((long long)n != (long long)cm.last_key.nx * cm.last_key.local_rows) return invalid("rt_debug_set_cost_map: n is not the last ranked frame's local pixel count");
    RT_TRY(use_device(s->device));
    if (s->frame_pending) RT_TRY(rt_frame_finish(s, nullptr));
    std::vector<unsigned int> words((size_t)n);
    unsigned long long total = 0;
    for (size_t k = 0; k < (size_t)n; ++k) { words[k] = in[k] & 0x7FFFFFFFu; total += words[k]; }
    cm.valid = false;
    RT_TRY(cm.grow((size_t)n));
    HIPCHK(hipMemcpy(cm.d, words.data(), (size_t)n * sizeof(unsigned int), hipMemcpyHostToDevice));
    cm.key = cm.last_key; cm.scene_epoch = s->scene_epoch; cm.opt_epoch = g_opt_epoch; cm.total = total; cm.valid = true;
    return RT_OK;
}

rt_status rt_debug_rank_info(rt_scene* s, uint32_t* out13) {
    if (!s) return invalid("rt_debug_rank_info: null scene");
    if (!out13) return invalid("rt_debug_rank_info: null argument");
    if (!s->plan.ranked || !s->d_rank) return invalid("rt_debug_rank_info: the scene's last frame was not ranked");
    RT_TRY(use_device(s->device));
    if (s->frame_pending) HIPCHK(hipStreamSynchronize(s->pending_stream));
    HIPCHK(hipMemcpy(out13, s->d_rank, sizeof(rt_rank_info), hipMemcpyDeviceToHost));
    return RT_OK;
}

// The tier kernel's room as rt_render plans it for this scene under the current options (diagnostics, every build;
// tests/test_kernel_matrix.py): plan_frame's tier_room -- out4 = fits, lds_scene (which instantiation of the tier kernel a tier or
// tail launch takes), the LDS image's bytes and the tail launch's grid.  The room depends on the scene, the device and the
// options, not on the frame, so the plan is made for the smallest ranked frame (64 tiles of 8 x 8 pixels).  Host only: no HIP
// call, nothing launched, the scene untouched; a plan the options make impossible is refused as rt_render refuses it.
rt_status rt_debug_tier_room(rt_scene* s, int32_t* out4) {
    if (!s) return invalid("rt_debug_tier_room: null scene");
    if (!out4) return invalid("rt_debug_tier_room: null argument");
    rt_frame_desc f;
    memset(&f, 0, sizeof(f));
    f.nx = f.ny = 64; f.ns = 1; f.gamma = 1.0f; f.tile_rows = 64; f.tile_stride = 1;
    const frame_geometry g = {64, 8, 8, 64u * 64u, 64u * 64u};
    const cost_map_view view = {false, false, cost_map_key(), 0ull, 0ull, 0ull, 0ull};
    frame_plan plan;
    const char* why = nullptr;
    if (plan_frame(plan_facts_of(s), g_opt, f, g, {false, 0, 0}, view, plan, why) != RT_OK) return invalid(why);
    out4[0] = plan.room.fits ? 1 : 0; out4[1] = plan.room.lds_scene; out4[2] = (int32_t)plan.room.lds; out4[3] = (int32_t)plan.room.tail_grid;
    return RT_OK;
}

// The passes of the last adaptive frame (diagnostics, tools/adaptive_sweep.py): per pass 5 values -- route (0 main kernel,
// 1 tier kernel), active pixels, sample_begin, sample_end, device ms (x1000) of the render launch.  Returns the number of passes.
int32_t rt_debug_adaptive_passes(const rt_scene* s, long long* out, int32_t cap) {
    if (!s) return -1;
    const int32_t np = (int32_t)s->adapt_ms.size();
    for (int32_t k = 0; k < np && k < cap; ++k) {
        for (int c = 0; c < 4; ++c) out[5 * k + c] = s->adapt_log[4 * k + c];
        out[5 * k + 4] = (long long)llround((double)s->adapt_ms[k] * 1000.0);
    }
    return np;
}

}  // extern "C"
