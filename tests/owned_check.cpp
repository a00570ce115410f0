// The owning device buffer (csrc/rt_owned.h) on its own, over a counting fake allocator that can be told to fail its n-th
// call: every expected value below is written out by hand.  tests/test_owned_host.py builds this with
// -fsanitize=address,undefined and runs it; no HIP, no device.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "rt_owned.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// malloc and free, counted; call number `fail_at` of allocate (counted from 1) fails with status 2 and allocates nothing
struct fake_memory {
    static int allocs, frees, calls, fail_at;
    static size_t last_bytes;
    static int allocate(void** p, size_t bytes) {
        last_bytes = bytes;
        if (++calls == fail_at) return 2;
        *p = std::malloc(bytes);
        ++allocs;
        return 0;
    }
    static void release(void* p) { std::free(p); ++frees; }
    static int live() { return allocs - frees; }
};
int fake_memory::allocs = 0, fake_memory::frees = 0, fake_memory::calls = 0, fake_memory::fail_at = 0;
size_t fake_memory::last_bytes = 0;
typedef owned<double, fake_memory> buffer;

int main() {
    {   // ---- grow: below the capacity nothing, above it one free and then one allocation
        buffer b;
        CHECK(b.get() == nullptr && b.capacity() == 0);
        CHECK(b.grow(0) == 0 && fake_memory::calls == 0 && b.get() == nullptr);      // nothing needed, nothing held
        CHECK(b.grow(10) == 0);
        CHECK(fake_memory::allocs == 1 && fake_memory::frees == 0 && fake_memory::last_bytes == 80);
        CHECK(b.get() != nullptr && b.capacity() == 10);
        double* const first = b.get();
        b[9] = 1.0;                                                                   // (the whole room is there)
        CHECK(b.grow(10) == 0 && b.grow(3) == 0 && b.grow(0) == 0);
        CHECK(fake_memory::allocs == 1 && fake_memory::frees == 0 && b.get() == first && b.capacity() == 10);
        CHECK(b.grow(11) == 0);
        CHECK(fake_memory::allocs == 2 && fake_memory::frees == 1 && fake_memory::last_bytes == 88 && b.capacity() == 11);
        b[10] = 2.0;
        double* as_pointer = b;                                                       // converts to what it holds
        CHECK(as_pointer == b.get() && fake_memory::live() == 1);
    }
    CHECK(fake_memory::allocs == 2 && fake_memory::frees == 2);                       // the destructor freed the second

    {   // ---- a failed grow leaves the buffer empty, and a later one succeeds
        buffer b;
        CHECK(b.grow(4) == 0 && fake_memory::allocs == 3);
        fake_memory::fail_at = fake_memory::calls + 1;
        CHECK(b.grow(8) == 2);
        CHECK(b.get() == nullptr && b.capacity() == 0);
        CHECK(fake_memory::allocs == 3 && fake_memory::frees == 3);                   // what it held went before the attempt
        CHECK(b.grow(2) == 0);                                                        // (below the old capacity: allocated all the same)
        CHECK(fake_memory::allocs == 4 && b.get() != nullptr && b.capacity() == 2);
        fake_memory::fail_at = fake_memory::calls + 1;
        buffer empty;
        CHECK(empty.grow(1) == 2 && empty.get() == nullptr && empty.capacity() == 0 && fake_memory::frees == 3);
    }
    CHECK(fake_memory::allocs == 4 && fake_memory::frees == 4);

    {   // ---- moves leave the source empty and free nothing twice
        buffer a;
        CHECK(a.grow(5) == 0);
        double* const p = a.get();
        buffer b(std::move(a));
        CHECK(a.get() == nullptr && a.capacity() == 0 && b.get() == p && b.capacity() == 5);
        CHECK(fake_memory::allocs == 5 && fake_memory::frees == 4);
        buffer c;
        CHECK(c.grow(7) == 0 && fake_memory::allocs == 6);
        c = std::move(b);                                                             // frees c's own seven, takes b's five
        CHECK(fake_memory::frees == 5 && c.get() == p && c.capacity() == 5 && b.get() == nullptr && b.capacity() == 0);
        buffer& same = c;
        c = std::move(same);                                                          // onto itself: nothing happens
        CHECK(fake_memory::frees == 5 && c.get() == p && c.capacity() == 5);
        b = std::move(a);                                                             // empty onto empty
        CHECK(fake_memory::frees == 5 && b.get() == nullptr);
    }
    CHECK(fake_memory::allocs == 6 && fake_memory::frees == 6);

    {   // ---- release then adopt hands the allocation over without a free; adopt frees what the taker held
        buffer from, to;
        CHECK(from.grow(6) == 0 && to.grow(1) == 0 && fake_memory::allocs == 8);
        double* const p = from.get();
        double* const handed = from.release();
        CHECK(handed == p && from.get() == nullptr && from.capacity() == 0 && fake_memory::frees == 6);
        to.adopt(handed, 6);
        CHECK(fake_memory::frees == 7 && to.get() == p && to.capacity() == 6);         // the one free is of `to`'s old element
        to[5] = 3.0;
        buffer fresh;
        fresh.adopt(to.release(), 6);
        CHECK(fake_memory::frees == 7 && fresh.get() == p && fresh.capacity() == 6 && to.get() == nullptr);
        CHECK(fresh.grow(6) == 0 && fake_memory::allocs == 8);                         // the adopted capacity counts
        CHECK(fake_memory::live() == 1);
    }
    // ---- at the end every allocation made was freed exactly once
    CHECK(fake_memory::allocs == 8 && fake_memory::frees == 8 && fake_memory::live() == 0);
    CHECK(fake_memory::calls == 10);                                                  // eight allocations and two told to fail

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("owned ok\n");
    return 0;
}
