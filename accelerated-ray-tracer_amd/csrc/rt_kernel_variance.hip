// rt_kernel_variance.hip -- the batch-means kernel of rt_render_variance (include/rt_abi.h).
//
// A variance frame renders in B passes [c_{b-1}, c_b) over every pixel; the render passes (the main kernel, rt_abi.hip) only
// park pixels.  After each pass this kernel runs one lane per local pixel: it reads the pixel's parked colour sum, forms the
// float triple m_b the frame would hold at c_b samples exactly as store_pixel does, recovers the batch's own mean y_b of
// r + g + b from T_b - T_{b-1} and adds it to the pixel's running sums A = sum y, Q = sum y^2 -- 24 bytes per pixel, in double,
// in the order the header states.  After the last pass it writes the frame (store_pixel's own code, gamma by cr_pow) and the
// variance of the pixel's mean.  A pixel is touched by its own lane only: no atomics, no order between lanes.
#include "rt_device_funcs.h"

__global__ void __launch_bounds__(RT_VARIANCE_THREADS) rt_variance_kernel(rt_variance_params p) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= p.n_pixels) return;
    const rt_pixel_state st = p.state[pix];
    // the linear average at c samples: store_pixel's scaling (vec3::operator/=(float), vec3.cuh:145-153), gamma 1
    const float kk = (float)(1.0 / (double)(float)p.c);
    const f3 m = mk3(st.col[0] * kk, st.col[1] * kk, st.col[2] * kk);
    const double s = ((double)m.x + (double)m.y) + (double)m.z;
    const double T = (double)p.c * s;
    double* acc = p.acc + (size_t)pix * 3;
    double T_prev = 0.0, A = 0.0, Q = 0.0;
    if (!p.first) { T_prev = acc[0]; A = acc[1]; Q = acc[2]; }
    const double y = (T - T_prev) / (double)p.per;
    A = A + y;
    Q = Q + y * y;
    if (!p.last) {
        acc[0] = T; acc[1] = A; acc[2] = Q;
        return;
    }
    const double mu = A / (double)p.batches;
    double v = Q / (double)p.batches - mu * mu;
    v = (v > 0.0) ? v : 0.0;   // a NaN compares false: 0
    p.variance[pix] = (float)(v / (double)(p.batches - 1));
    rt_frame_params fp = {};   // store_pixel reads fb, nx, ns and gamma
    fp.fb = p.fb; fp.nx = p.nx; fp.ns = p.c; fp.gamma = p.gamma;
    const int lrow = (int)(pix / (uint32_t)p.nx), i = (int)(pix - (uint32_t)lrow * (uint32_t)p.nx);
    store_pixel(fp, i, lrow, mk3(st.col[0], st.col[1], st.col[2]));
}

hipError_t rt_launch_variance(const rt_variance_params& p, hipStream_t st) {
    if (p.n_pixels == 0u) return hipSuccess;
    const unsigned grid = (p.n_pixels + RT_VARIANCE_THREADS - 1u) / RT_VARIANCE_THREADS;
    hipLaunchKernelGGL(rt_variance_kernel, dim3(grid), dim3(RT_VARIANCE_THREADS), 0, st, p);
    return hipGetLastError();
}
