// rt_handoff_order.h -- ordering the tail hand-off queue (rt_rank.hip; rt_abi.hip "tail").
//
// The main kernel's lanes push (next sample << 32 | pixel) to the hand-off queue in whatever order they reach a sample boundary;
// the tail launch's waves pull entries from its head.  Between the two, on the same stream, two small kernels copy the queue
// into a second buffer with the entries that have the most work left first, so that the tail is dealt like every other queue
// of the frame: longest first.  Scheduling only -- which wave finishes a pixel never changes the pixel.
//
// Remaining work of an entry (the key, 64-bit):
//     key = (sample_end - next) * (rays so far + 1) / (samples done + 1)
// with "rays so far" the low 31 bits of the parked cost and "samples done" = next - cost_begin, the samples that cost covers.
// The keys are bucketed on a fixed logarithmic scale, RT_HANDOFF_SUB_BITS bits below the leading one (four buckets an octave),
// so no pass for the maximum is needed: bucket 0 holds key 0, bucket 1 + 4 e + m the keys with leading bit e and next two bits m.
// Within a bucket the order is whatever the atomics give.
//
// The queue is copied through unordered when it holds fewer than min_items entries (two per tail wave: nothing to balance) or
// more than max_items (RT_HANDOFF_ORDER_MAX_PER_WAVE per tail wave: with that many entries a wave the tail is bound by
// throughput, the last entry a wave takes is 1/32 of its load, and the sort only costs time).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device.h"

enum { RT_HANDOFF_SUB_BITS = 2,
       RT_HANDOFF_BUCKETS = 1 + 64 * (1 << RT_HANDOFF_SUB_BITS),   // 257
       RT_HANDOFF_ORDER_THREADS = 256,
       RT_HANDOFF_ORDER_MIN_PER_WAVE = 2,
       RT_HANDOFF_ORDER_MAX_PER_WAVE = 32 };

struct rt_handoff_order_params {
    const unsigned long long* queue;     // the main kernel's queue, push order
    unsigned long long* ordered;         // out: the same entries, most remaining work first (or a plain copy)
    const rt_pixel_state* state;         // handoff_state: .cost of an entry's pixel = its rays so far
    const unsigned int* pushed;          // work_counter + RT_WC_PUSHED: entries pushed (may exceed cap: those were not stored)
    // scratch, rt_handoff_order_scratch_words(max_items) words, the first RT_HANDOFF_BUCKETS of them ZERO before the launch:
    // [0, BUCKETS) entries per bucket, then per workgroup of the histogram kernel where its entries start within each bucket
    unsigned int* scratch;
    uint32_t cap;                        // entries the queue holds
    uint32_t min_items, max_items;       // ordered only for min_items <= count <= max_items
    int32_t cost_begin;                  // first sample the parked costs cover
    int32_t sample_end;
};

inline size_t rt_handoff_order_scratch_words(uint32_t max_items) {
    const size_t wgs = ((size_t)max_items + RT_HANDOFF_ORDER_THREADS - 1) / RT_HANDOFF_ORDER_THREADS;
    return (size_t)RT_HANDOFF_BUCKETS * (wgs + 1);
}
// the ordering kernels of one tail launch, enqueued on `st` (no host synchronisation); max_items <= cap
hipError_t rt_launch_handoff_order(const rt_handoff_order_params& hp, hipStream_t st);
