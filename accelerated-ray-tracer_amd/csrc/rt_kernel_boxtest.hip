// rt_kernel_boxtest.hip -- rt_debug_box_tests (include/rt_abi.h): the three box tests of rt_device_funcs.h, each run as the
// render kernels run it, on caller-supplied boxes and rays.  One case per thread; a test seam (tests/test_box_tests.py), never
// on a frame's path.  Internal to librt_mi355x.so; launched by rt_abi.hip.
#include "rt_device_funcs.h"

namespace {

__global__ void __launch_bounds__(256) rt_box_tests_kernel(rt_box_test_params bp) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= bp.n) return;
    // the node record as the walk reads it: bmin + a link word, bmax + a link word (the tests do not read the links)
    const float4 a = make_float4(bp.bmin[3 * i], bp.bmin[3 * i + 1], bp.bmin[3 * i + 2], 0.0f);
    const float4 b = make_float4(bp.bmax[3 * i], bp.bmax[3 * i + 1], bp.bmax[3 * i + 2], 0.0f);
    const f3 o = ld3(bp.origins + 3 * i), d = ld3(bp.directions + 3 * i);
    const float tmin = bp.tmin[i], tmax = bp.tmax[i];
    // a ray's box-test terms as stage F of the main kernel sets them up
    const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    const bool finite_inv = inv_is_finite(inv) && loose_ok(inv, o, bp.bound);
    const LooseRay lr = loose_setup(inv, o, bp.bound);
    uint8_t* f = bp.flags + 4 * (size_t)i;
    f[0] = slab_test(a, b, o, inv, tmin, tmax) ? 1 : 0;
    f[1] = slab_test_finite(a, b, o, inv, tmin, tmax) ? 1 : 0;
    f[2] = slab_test_loose(a, b, inv, lr, tmin, tmax) ? 1 : 0;
    f[3] = finite_inv ? 1 : 0;
}

}  // namespace

hipError_t rt_launch_box_tests(const rt_box_test_params& bp, hipStream_t st) {
    hipLaunchKernelGGL(rt_box_tests_kernel, dim3((unsigned)((bp.n + 255) / 256)), dim3(256), 0, st, bp);
    return hipGetLastError();
}
