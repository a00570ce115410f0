// rt_call_buffers.h -- the buffer table of an image-space entry point (rt_abi.hip: rt_render_aov*, rt_denoise*, rt_upscale,
// rt_reproject*): the record of one caller buffer, whether two of them share a byte, and how the device images of host buffers
// are cut out of the call's one allocation (call_memory, rt_host.h).  Plain host code without a HIP call, so that it also builds into a stand-alone
// program (tests/test_call_buffers_host.py runs it under the address and undefined-behaviour sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>

// one allocation cut into 256-byte-rounded pieces, in the order they are taken
struct call_pieces {
    static size_t rounded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    static char* take(char*& at, size_t bytes) { char* piece = at; at += rounded(bytes); return piece; }
};

// a pointer a caller hands to a kernel: null, or `bytes` of memory aligned to `align` bytes; `what` names it in refusals
struct traced_ptr { const void* p; size_t bytes; const char* what; unsigned align; };

// ... and what an image-space call does with it: a BUF_WORKSPACE is the caller's device memory in either mode; it is neither
// staged nor copied
enum buffer_role { BUF_INPUT, BUF_OUTPUT, BUF_WORKSPACE };
struct call_buffer : traced_ptr { buffer_role role; };

// whether two buffers share a byte (a null buffer shares none)
inline bool share_a_byte(const traced_ptr& a, const traced_ptr& b) {
    const uintptr_t pa = (uintptr_t)a.p, pb = (uintptr_t)b.p;
    return a.p && b.p && pa < pb + b.bytes && pb < pa + a.bytes;
}

// The device images of the inputs and outputs of `table` for which used(k), in table order, behind `lead` bytes that the caller
// keeps for itself: the size of the allocation, and the images' places in it (dev[k]; the other entries of dev are left as they are).
template <class Table, class Used> size_t staged_bytes(const Table& table, Used used, size_t lead) {
    size_t total = lead;
    int k = 0;
    for (const call_buffer& b : table) { if (b.role != BUF_WORKSPACE && used(k)) total += call_pieces::rounded(b.bytes); ++k; }
    return total;
}
template <class Table, class Used> void place_staged(const Table& table, Used used, char* base, size_t lead, const void** dev) {
    char* at = base + lead;
    int k = 0;
    for (const call_buffer& b : table) { if (b.role != BUF_WORKSPACE && used(k)) dev[k] = call_pieces::take(at, b.bytes); ++k; }
}
