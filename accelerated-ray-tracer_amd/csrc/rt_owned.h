// rt_owned.h -- a device buffer that frees itself: what struct rt_scene, rt_progressive and call_memory (rt_host.h) hold in
// place of a raw pointer, a capacity field and a line in a destroy function.  The memory comes from `Memory`: hip_memory where
// this header is included after the HIP runtime header, a counting fake in tests/owned_check.cpp, which
// tests/test_owned_host.py runs under the address and undefined-behaviour sanitizers.  No HIP call of its own.
#pragma once
#include <cstddef>

#ifdef HIP_INCLUDE_HIP_HIP_RUNTIME_API_H
struct hip_memory {
    static int allocate(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }   // 0 (hipSuccess) or the hipError_t
    static void release(void* p) { (void)hipFree(p); }
};
#else
struct hip_memory;
#endif

// `capacity` elements of T at `get()` (which an owned<T> also converts to), or null and 0.  Move-only.
template <class T, class Memory = hip_memory>
class owned {
    T* p_ = nullptr;
    size_t capacity_ = 0;
public:
    owned() = default;
    owned(const owned&) = delete;
    owned& operator=(const owned&) = delete;
    owned(owned&& o) noexcept : p_(o.p_), capacity_(o.capacity_) { o.p_ = nullptr; o.capacity_ = 0; }
    owned& operator=(owned&& o) noexcept {
        if (this != &o) { const size_t c = o.capacity_; adopt(o.release(), c); }
        return *this;
    }
    ~owned() { adopt(nullptr, 0); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return capacity_; }
    // Room for `need` elements: nothing to do when it is there already; else what is held is freed and the room allocated anew
    // (the contents are not kept).  Returns Memory's status, 0 for success; after a failure the buffer is empty.
    int grow(size_t need) {
        if (capacity_ >= need) return 0;
        adopt(nullptr, 0);
        void* p = nullptr;
        const int status = Memory::allocate(&p, need * sizeof(T));
        if (status == 0) adopt(static_cast<T*>(p), need);
        return status;
    }
    // gives up what is held without freeing it; takes over an allocation of `capacity` elements made elsewhere (what is held is freed)
    T* release() { T* p = p_; p_ = nullptr; capacity_ = 0; return p; }
    void adopt(T* p, size_t capacity) {
        if (p_) Memory::release(p_);
        p_ = p; capacity_ = capacity;
    }
};
