// rt_launch.h -- the host side of a kernel launch, shared by every unit that launches with dynamic LDS: the opt-in above
// 64 KiB, the launch and the occupancy query, over a kernel function pointer.  All instantiations of one kernel template have
// one function type, so a unit picks the instantiation as a pointer and hands it here.  Internal to librt_mi355x.so.
#pragma once
#include <hip/hip_runtime.h>

// a kernel may use more than 64 KiB of dynamic LDS only after this
template <typename K>
hipError_t rt_lds_opt_in(K* kernel, size_t lds) {
    if (lds <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// the launch's hipError_t, a failed opt-in first
template <typename K, typename... A>
hipError_t rt_launch_kernel(K* kernel, dim3 threads, dim3 grid, size_t lds, hipStream_t st, const A&... args) {
    const hipError_t e = rt_lds_opt_in(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, threads, lds, st, args...);
    return hipGetLastError();
}

// workgroups per CU of `kernel` with `threads` lanes and `lds` bytes of dynamic LDS each
template <typename K>
hipError_t rt_kernel_occupancy(K* kernel, int threads, size_t lds, int* blocks) {
    const hipError_t e = rt_lds_opt_in(kernel, lds);
    if (e != hipSuccess) return e;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void*>(kernel), threads, lds);
}
