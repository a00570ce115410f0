// The buffer table of the image-space entries (csrc/rt_call_buffers.h) on its own: every expected value below is written out
// by hand.  tests/test_call_buffers_host.py builds this with -fsanitize=address,undefined and runs it; no HIP, no device.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_call_buffers.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static call_buffer at(uintptr_t p, size_t bytes, buffer_role role = BUF_INPUT) {
    return call_buffer{{reinterpret_cast<const void*>(p), bytes, "x", 4}, role};
}

int main() {
    // ---- share_a_byte: [p, p + bytes) against [q, q + bytes)
    CHECK(share_a_byte(at(0x1000, 16), at(0x1000, 16)));            // equal
    CHECK(share_a_byte(at(0x1000, 64), at(0x1010, 16)));            // nested, both ways round
    CHECK(share_a_byte(at(0x1010, 16), at(0x1000, 64)));
    CHECK(share_a_byte(at(0x1000, 17), at(0x1010, 16)));            // the last byte of one is the first of the other
    CHECK(share_a_byte(at(0x1010, 16), at(0x1000, 17)));
    CHECK(!share_a_byte(at(0x1000, 16), at(0x1010, 16)));           // adjacent: one ends where the other begins
    CHECK(!share_a_byte(at(0x1010, 16), at(0x1000, 16)));
    CHECK(!share_a_byte(at(0x1000, 16), at(0x2000, 16)));           // apart
    CHECK(!share_a_byte(at(0, 16), at(0, 16)));                     // null shares nothing, not even with null
    CHECK(!share_a_byte(at(0, 0x2000), at(0x1000, 16)));
    CHECK(!share_a_byte(at(0x1000, 16), at(0, 0x2000)));
    CHECK(!share_a_byte(at(0x1000, 0), at(0x1000, 16)));            // an empty buffer at the start of another holds no byte
    CHECK(share_a_byte(at(0x1008, 0), at(0x1000, 16)) == true);     // (inside one it compares as the interval test does: strictly inside)

    // ---- rounded and take: 256-byte pieces in the order taken
    CHECK(call_pieces::rounded(0) == 0);
    CHECK(call_pieces::rounded(1) == 256);
    CHECK(call_pieces::rounded(256) == 256);
    CHECK(call_pieces::rounded(257) == 512);
    CHECK(call_pieces::rounded(11520) == 11520);                    // 48 x 20 x 3 floats
    CHECK(call_pieces::rounded(3840) == 3840);                      // 48 x 20 floats
    CHECK(call_pieces::rounded(12) == 256);                         // a 1 x 1 frame
    std::vector<char> memory(4096);
    char* const base = memory.data();
    char* cursor = base;
    CHECK(call_pieces::take(cursor, 12) == base && cursor == base + 256);
    CHECK(call_pieces::take(cursor, 300) == base + 256 && cursor == base + 768);
    CHECK(call_pieces::take(cursor, 256) == base + 768 && cursor == base + 1024);

    // ---- staged_bytes and place_staged: a denoiser-like table (a caller's workspace, which is never staged; an absent guide; an output
    // that is its input), behind 1024 leading bytes
    enum { COLOR, ALBEDO, NORMAL, OUT, WORKSPACE, VARIANCE_OUT, N };
    const call_buffer table[N] = {at(0x10000, 36), at(0x20000, 36), at(0, 36), at(0x10000, 36, BUF_OUTPUT), at(0x40000, 3072, BUF_WORKSPACE),
                                  at(0x30000, 12, BUF_OUTPUT)};
    auto staged = [&](int k) { return table[k].p != nullptr && k != OUT; };
    CHECK(staged_bytes(table, staged, 1024) == 1024 + 3 * 256);     // color, albedo, variance_out: 36 -> 256, 36 -> 256, 12 -> 256
    CHECK(staged_bytes(table, staged, 0) == 768);
    CHECK(staged_bytes(table, [](int) { return false; }, 1024) == 1024);
    CHECK(staged_bytes(table, [](int) { return true; }, 0) == 4 * 256 + 256);             // (not the workspace's 3072, whatever `used` says)
    const char marker = 0;
    const void* dev[N];
    for (int k = 0; k < N; ++k) dev[k] = &marker;
    place_staged(table, staged, base, 1024, dev);
    CHECK(dev[COLOR] == base + 1024);                               // table order, each piece behind the one before
    CHECK(dev[ALBEDO] == base + 1280);
    CHECK(dev[VARIANCE_OUT] == base + 1536);
    CHECK(dev[NORMAL] == &marker && dev[OUT] == &marker && dev[WORKSPACE] == &marker);   // what is not staged is left alone
    // every placed piece lies inside the allocation staged_bytes asked for, and can be written over its full rounded size
    std::vector<char> exact(staged_bytes(table, staged, 1024));
    place_staged(table, staged, exact.data(), 1024, dev);
    for (int k : {(int)COLOR, (int)ALBEDO, (int)VARIANCE_OUT}) {
        char* piece = const_cast<char*>(static_cast<const char*>(dev[k]));
        for (size_t b = 0; b < call_pieces::rounded(table[k].bytes); ++b) piece[b] = 1;
    }
    CHECK(static_cast<const char*>(dev[VARIANCE_OUT]) + 256 == exact.data() + exact.size());

    // sizes that are multiples of 256 already, and an upscaler-like table where everything given is staged
    const call_buffer frames[3] = {at(0x1000, 11520), at(0, 11520), at(0x9000, 3840, BUF_OUTPUT)};
    auto given = [&](int k) { return frames[k].p != nullptr; };
    CHECK(staged_bytes(frames, given, 0) == 11520 + 3840);
    const void* where[3] = {nullptr, nullptr, nullptr};
    place_staged(frames, given, base, 0, where);
    CHECK(where[0] == base && where[1] == nullptr && where[2] == base + 11520);

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("call buffers ok\n");
    return 0;
}
