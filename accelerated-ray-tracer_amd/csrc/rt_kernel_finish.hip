// rt_kernel_finish.hip -- the finishing pass of rt_render and rt_render_window.
//
// The main kernel and the tier kernel store each finished pixel's colour sum, three floats, where the reference's loop nest
// (main.cu:128-132) stores the pixel.  This kernel runs once over the frame's local rows, one lane per float, and does what
// store_pixel does to that sum: the scaling by k = (float)(1.0 / (double)(float)ns) (vec3::operator/=(float),
// vec3.cuh:145-153), then apply_gamma with the correctly rounded cr_pow.  Same operations on the same values, so the frame is
// store_pixel's bit for bit -- with every lane of a wave busy, where the end of a pixel inside the render kernels is an event
// of one lane in 64.  A value is read and written by its own lane only, in place.
#include "rt_device_funcs.h"

__global__ void __launch_bounds__(RT_FINISH_THREADS) rt_finish_kernel(float* fb, size_t floats, int32_t ns, float gamma) {
    const float k = (float)(1.0 / (double)(float)ns);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t at = (size_t)blockIdx.x * blockDim.x + threadIdx.x; at < floats; at += stride) fb[at] = apply_gamma(fb[at] * k, gamma);
}

hipError_t rt_launch_finish(float* fb, size_t floats, int32_t ns, float gamma, hipStream_t st) {
    if (floats == 0) return hipSuccess;
    const size_t blocks = (floats + RT_FINISH_THREADS - 1) / RT_FINISH_THREADS;
    const unsigned grid = (unsigned)(blocks < (size_t)(1u << 20) ? blocks : (size_t)(1u << 20));
    hipLaunchKernelGGL(rt_finish_kernel, dim3(grid), dim3(RT_FINISH_THREADS), 0, st, fb, floats, ns, gamma);
    return hipGetLastError();
}
