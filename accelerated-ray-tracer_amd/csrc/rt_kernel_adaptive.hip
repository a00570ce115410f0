// rt_kernel_adaptive.hip -- the decision and compaction kernel of rt_render_adaptive (include/rt_abi.h).
//
// An adaptive frame renders in passes between checkpoints c_k = min_spp * 2^k; the render passes (the main kernel over a
// pixel list, or the tier kernel's tail mode over a queue: rt_abi.hip) only park pixels.  After each pass this kernel runs
// one lane per pixel of that pass: it reads the pixel's parked colour sum, forms its linear average `a` at the checkpoint
// exactly as store_pixel does, and compares it with the average `h` it saved at the previous checkpoint.  A converged pixel
// is written to the frame (store_pixel's own code, gamma by cr_pow) and to the sample-count map and is dropped; an active
// one saves `a` as its next `h` and is appended to the next pass's pixel list and queue.
#include "rt_device_funcs.h"

namespace {

// one wave-aggregated append per wave: ballot, mbcnt, one atomic.  A wave's kept pixels stay together and in lane order.
DEV void append_active(const rt_adaptive_params& p, bool keep, uint32_t pix) {
    const unsigned long long m = __ballot(keep);
    if (m == 0ull) return;
    uint32_t base = 0u;
    if ((threadIdx.x & 63u) == 0u) base = atomicAdd(p.count_out, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (keep) {
        p.list_out[base + rank] = pix;
        p.queue_out[base + rank] = ((unsigned long long)(uint32_t)p.n << 32) | (unsigned long long)pix;
    }
}

}  // namespace

__global__ void __launch_bounds__(RT_ADAPTIVE_THREADS) rt_adaptive_decide_kernel(rt_adaptive_params p) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = k < p.n_in;
    const uint32_t pix = valid ? (p.list_in ? p.list_in[k] : k) : 0u;
    bool keep = false;
    if (valid) {
        const rt_pixel_state st = p.state[pix];
        // the linear average at n samples: store_pixel's scaling (vec3::operator/=(float), vec3.cuh:145-153), gamma 1
        const float kk = (float)(1.0 / (double)(float)p.n);
        const f3 a = mk3(st.col[0] * kk, st.col[1] * kk, st.col[2] * kk);
        float* h = p.half + (size_t)pix * 3;
        if (p.mode == RT_ADAPTIVE_SNAPSHOT) {
            h[0] = a.x; h[1] = a.y; h[2] = a.z;
        } else {
            bool done = true;   // RT_ADAPTIVE_FINAL: every pixel still active stops at max_spp
            if (p.mode == RT_ADAPTIVE_DECIDE) {
                // the criterion of include/rt_abi.h, in double, left to right; a NaN in d never converges
                const double d = fabs((double)a.x - (double)h[0]) + fabs((double)a.y - (double)h[1]) + fabs((double)a.z - (double)h[2]);
                const double s = (double)a.x + (double)a.y + (double)a.z;
                done = p.threshold >= 0.0f && d <= (double)p.threshold * (s + (double)p.floor);
            }
            if (done) {
                rt_frame_params fp;
                fp.fb = p.fb; fp.nx = p.nx; fp.ns = p.n; fp.gamma = p.gamma;
                const int lrow = (int)(pix / (uint32_t)p.nx), i = (int)(pix - (uint32_t)lrow * (uint32_t)p.nx);
                store_pixel(fp, i, lrow, mk3(st.col[0], st.col[1], st.col[2]));
                if (p.spp) p.spp[pix] = p.n;
            } else {
                h[0] = a.x; h[1] = a.y; h[2] = a.z;
                keep = true;
            }
        }
    }
    if (p.mode == RT_ADAPTIVE_DECIDE) append_active(p, keep, pix);
}

hipError_t rt_launch_adaptive(const rt_adaptive_params& p, hipStream_t st) {
    if (p.n_in == 0u) return hipSuccess;
    const unsigned grid = (p.n_in + RT_ADAPTIVE_THREADS - 1u) / RT_ADAPTIVE_THREADS;
    hipLaunchKernelGGL(rt_adaptive_decide_kernel, dim3(grid), dim3(RT_ADAPTIVE_THREADS), 0, st, p);
    return hipGetLastError();
}
