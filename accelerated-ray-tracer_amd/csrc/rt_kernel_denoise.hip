// rt_kernel_denoise.hip -- rt_denoise and rt_denoise_variance: the edge-avoiding a-trous filter of include/rt_abi.h
// ("denoiser"), gfx950.
//
// Two passes.  The pack pass turns the planar inputs into two 16-byte records per pixel (colour: x_0.rgb and a fourth float;
// guide: N.xyz, Z), so that a tap is two dwordx4 loads.  The iteration runs once per iteration k on workgroups of 256
// threads = four waves on 8x8 pixels each = a 16x16 tile, one pixel per lane in registers; it reads x_k and writes
// x_{k+1} (or, in the last iteration, the planar output, remodulated).  Both modes run one body, denoise_iteration, specialised
// on which guide factors are on, on the last factor of a tap (denoise_mode) and on how the taps are fetched:
//   staged  the tile and its halo of 2 s pixels go to LDS once, and the 25 taps of every pixel are LDS reads;
//   direct  every tap is read through L1/L2.
// Which one an iteration gets is the host's choice (rt_abi.hip, option "denoise_lds"); the arithmetic is the
// same statements in the same order in both, so the choice changes no bit.
//
// The record's fourth float is the colour sum (x.r + x.g) + x.b, which only the colour factor reads, or in the variance mode
// the pixel's variance v_k, which its pack pass pre-blurs 3x3 from the planar input and every iteration filters with the
// squared weights.  The variance mode's arguments are a second block that only its entry points take: the
// body sees it as a type, and the other modes pass an empty one.
//
// Bounds: a tap outside the image is skipped by an index test before any address is formed; the staging loop loads only
// the records inside the image, and a tap that passes the index test is inside the image and inside the staged window by
// construction (|offset| <= 2 s), so no slot is read that was not written.  No address depends on pixel data.
#include "rt_device.h"
#include "rt_filter.h"
#include "rt_launch.h"

namespace {

using namespace rt_filter;

__global__ __launch_bounds__(RT_DENOISE_THREADS) void rt_denoise_pack_kernel(rt_denoise_params dp, int guide) {
    const size_t n = (size_t)dp.nx * dp.ny;
    const size_t p = (size_t)blockIdx.x * RT_DENOISE_THREADS + threadIdx.x;
    if (p >= n) return;
    const float3 x = demodulated(dp.color, dp.albedo, dp.demodulate, p);
    dp.x_out[p] = make_float4(x.x, x.y, x.z, (x.x + x.y) + x.z);
    if (guide) dp.guide[p] = guide_record(dp.normal != nullptr, dp.depth != nullptr, dp.normal, dp.depth, p);
}

// the last factor of a tap, and with it what the record's fourth float is
enum denoise_mode { NO_COLOR, COLOR, VARIANCE };
struct no_variance_params {};   // the second argument block of the modes that have none

// one iteration for the lane's pixel; DV is rt_denoise_variance_params in the variance mode
// (dp by value, as the entry points hold it, and dv by reference: of the four combinations the one in which no mode runs slower
// than it did as a kernel of its own -- with dp by reference the staged all-guides kernels grew by 15 and 19 instructions and the
// variance mode at denoise_lds 1 ran 0.6 % slower; profiles/filter_shared_mi355x.jsonl)
template <bool NRM, bool DEP, denoise_mode MODE, bool STAGED, class DV>
__device__ __forceinline__ void denoise_iteration(const rt_denoise_params dp, const DV& dv) {
    extern __shared__ float4 lds[];
    constexpr bool GUIDE = NRM || DEP;
    const int tid = threadIdx.x;
    const int nx = dp.nx, ny = dp.ny, s = dp.step;
    const tile_pixel tile = tile_mapping(dp.tiles_x);
    const unsigned i = tile.i, j = tile.j;

    const int lw = TILE + 4 * s, stride = rt_denoise_lds_stride(s);
    const unsigned ox = (unsigned)tile.x0 - 2u * s, oy = (unsigned)tile.y0 - 2u * s;     // image coordinates of LDS slot (0, 0)
    const float4* lc = lds;
    const float4* lg = lds + stride * lw;
    if (STAGED) {
        for (int t = tid; t < lw * lw; t += RT_DENOISE_THREADS) {
            const int ly = t / lw, lx = t - ly * lw;
            const unsigned gx = ox + lx, gy = oy + ly;
            if (gx < (unsigned)nx && gy < (unsigned)ny) {
                const size_t q = (size_t)gy * nx + gx;
                lds[ly * stride + lx] = dp.x_in[q];
                if (GUIDE) lds[stride * lw + ly * stride + lx] = dp.guide[q];
            }
        }
        __syncthreads();
    }
    if (i >= (unsigned)nx || j >= (unsigned)ny) return;

    const size_t p = (size_t)j * nx + i;
    float4 xp, gp = make_float4(0.f, 0.f, 0.f, 0.f);
    if (STAGED) {
        const int c = (int)(j - oy) * stride + (int)(i - ox);
        xp = lc[c];
        if (GUIDE) gp = lg[c];
    } else {
        xp = dp.x_in[p];
        if (GUIDE) gp = dp.guide[p];
    }

    const float H[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sigma2 = 0.f;
    if constexpr (MODE == VARIANCE) sigma2 = dv.sigma_variance * dv.sigma_variance;
    float W = 0.f, Sr = 0.f, Sg = 0.f, Sb = 0.f, Sv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const unsigned qy = j + (unsigned)(s * dy);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const unsigned qx = i + (unsigned)(s * dx);
            if (qx >= (unsigned)nx || qy >= (unsigned)ny) continue;
            float4 xq, gq = make_float4(0.f, 0.f, 0.f, 0.f);
            if (STAGED) {
                const int c = (int)(qy - oy) * stride + (int)(qx - ox);
                xq = lc[c];
                if (GUIDE) gq = lg[c];
            } else {
                const size_t q = (size_t)qy * nx + qx;
                xq = dp.x_in[q];
                if (GUIDE) gq = dp.guide[q];
            }
            float w = H[dy + 2] * H[dx + 2];
            if (dx != 0 || dy != 0) {
                if (NRM) w = w * normal_factor(gp, gq, dp.normal_sharpness);
                if (DEP) w = w * depth_factor(gp, gq, dp.sigma_depth);
                if constexpr (MODE == COLOR) {
                    const float d1 = (fabsf(xp.x - xq.x) + fabsf(xp.y - xq.y)) + fabsf(xp.z - xq.z);
                    const float den = dp.sigma_color_k * ((xp.w + xq.w) + dp.color_floor);
                    const float r = d1 / den;
                    const float t = fmaxf(1.f - r, 0.f);
                    w = w * (t * t);
                }
                if constexpr (MODE == VARIANCE) {   // the colour difference against what the two pixels' noise explains
                    const float d1 = (fabsf(xp.x - xq.x) + fabsf(xp.y - xq.y)) + fabsf(xp.z - xq.z);
                    const float den = sigma2 * (xp.w + xq.w) + dv.variance_floor;
                    const float r = (d1 * d1) / den;
                    const float t = fmaxf(1.f - r, 0.f);
                    w = w * (t * t);
                }
            }
            W = W + w;
            Sr = Sr + w * xq.x;
            Sg = Sg + w * xq.y;
            Sb = Sb + w * xq.z;
            if constexpr (MODE == VARIANCE) Sv = Sv + (w * w) * xq.w;
        }
    }
    float r = Sr / W, g = Sg / W, b = Sb / W, v = 0.f;
    if constexpr (MODE == VARIANCE) v = Sv / (W * W);
    if (!dp.last) {
        dp.x_out[p] = make_float4(r, g, b, MODE == VARIANCE ? v : (r + g) + b);
        return;
    }
    remodulate(dp.albedo, dp.demodulate, p, r, g, b);
    dp.out[3 * p] = r;
    dp.out[3 * p + 1] = g;
    dp.out[3 * p + 2] = b;
    if constexpr (MODE == VARIANCE) {
        if (dv.variance_out) {
            if (dp.demodulate) {
                const float t = variance_scale(dp.albedo, p);
                v = (v / t) / t;
            }
            dv.variance_out[p] = v;
        }
    }
}

template <bool NRM, bool DEP, bool COL, bool STAGED>
__global__ __launch_bounds__(RT_DENOISE_THREADS) void rt_denoise_kernel(rt_denoise_params dp) {
    denoise_iteration<NRM, DEP, COL ? COLOR : NO_COLOR, STAGED>(dp, no_variance_params{});
}

template <bool NRM, bool DEP, bool COL, bool STAGED>
hipError_t launch(const rt_denoise_params& dp, hipStream_t st) {
    const size_t lds = STAGED ? rt_denoise_lds_bytes(dp.step, NRM || DEP) : 0;
    const unsigned tiles_y = ((unsigned)dp.ny + TILE - 1) / TILE;
    return rt_launch_kernel(rt_denoise_kernel<NRM, DEP, COL, STAGED>, dim3(RT_DENOISE_THREADS), dim3((unsigned)dp.tiles_x * tiles_y), lds, st, dp);
}

template <bool NRM, bool DEP, bool COL>
hipError_t launch_staged(bool staged, const rt_denoise_params& dp, hipStream_t st) {
    return staged ? launch<NRM, DEP, COL, true>(dp, st) : launch<NRM, DEP, COL, false>(dp, st);
}
template <bool NRM, bool DEP>
hipError_t launch_color(bool color_on, bool staged, const rt_denoise_params& dp, hipStream_t st) {
    return color_on ? launch_staged<NRM, DEP, true>(staged, dp, st) : launch_staged<NRM, DEP, false>(staged, dp, st);
}

}  // namespace

hipError_t rt_launch_denoise_pack(const rt_denoise_params& dp, bool guide, hipStream_t st) {
    const size_t n = (size_t)dp.nx * dp.ny;
    hipLaunchKernelGGL(rt_denoise_pack_kernel, dim3((unsigned)((n + RT_DENOISE_THREADS - 1) / RT_DENOISE_THREADS)), dim3(RT_DENOISE_THREADS), 0, st, dp,
                       guide ? 1 : 0);
    return hipGetLastError();
}

hipError_t rt_launch_denoise(bool normal_on, bool depth_on, bool color_on, bool staged, const rt_denoise_params& dp, hipStream_t st) {
    if (normal_on) return depth_on ? launch_color<true, true>(color_on, staged, dp, st) : launch_color<true, false>(color_on, staged, dp, st);
    return depth_on ? launch_color<false, true>(color_on, staged, dp, st) : launch_color<false, false>(color_on, staged, dp, st);
}

// ---- the variance-guided mode (rt_denoise_variance) ----
namespace {

// the pack pass: x_0 and the guide record as rt_denoise_pack_kernel writes them, and in the colour record's fourth float
// v_0 = the 3x3 binomial pre-blur of u, straight from the planar inputs
template <bool GUIDE>
__global__ __launch_bounds__(RT_DENOISE_THREADS) void rt_denoise_pack_variance_kernel(rt_denoise_params dp, rt_denoise_variance_params dv) {
    const size_t n = (size_t)dp.nx * dp.ny;
    const size_t p = (size_t)blockIdx.x * RT_DENOISE_THREADS + threadIdx.x;
    if (p >= n) return;
    const float3 x = demodulated(dp.color, dp.albedo, dp.demodulate, p);
    // (coordinates are unsigned: -1 wraps and compares as out of the image)
    const unsigned j = (unsigned)(p / (size_t)dp.nx), i = (unsigned)(p - (size_t)j * dp.nx);
    const float G[3] = {0.25f, 0.5f, 0.25f};
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const unsigned qy = j + (unsigned)dy;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const unsigned qx = i + (unsigned)dx;
            if (qx >= (unsigned)dp.nx || qy >= (unsigned)dp.ny) continue;
            const size_t q = (size_t)qy * dp.nx + qx;
            float u = dv.variance[q];
            if (dp.demodulate) {
                const float t = variance_scale(dp.albedo, q);
                u = (u * t) * t;
            }
            const float w = G[dy + 1] * G[dx + 1];
            num = num + w * u;
            den = den + w;
        }
    }
    dp.x_out[p] = make_float4(x.x, x.y, x.z, num / den);
    if (GUIDE) dp.guide[p] = guide_record(dp.normal != nullptr, dp.depth != nullptr, dp.normal, dp.depth, p);
}

template <bool NRM, bool DEP, bool STAGED>
__global__ __launch_bounds__(RT_DENOISE_THREADS) void rt_denoise_variance_kernel(rt_denoise_params dp, rt_denoise_variance_params dv) {
    denoise_iteration<NRM, DEP, VARIANCE, STAGED>(dp, dv);
}

template <bool NRM, bool DEP, bool STAGED>
hipError_t launch_variance(const rt_denoise_params& dp, const rt_denoise_variance_params& dv, hipStream_t st) {
    const size_t lds = STAGED ? rt_denoise_lds_bytes(dp.step, NRM || DEP) : 0;
    const unsigned tiles_y = ((unsigned)dp.ny + TILE - 1) / TILE;
    return rt_launch_kernel(rt_denoise_variance_kernel<NRM, DEP, STAGED>, dim3(RT_DENOISE_THREADS), dim3((unsigned)dp.tiles_x * tiles_y), lds, st, dp, dv);
}
template <bool NRM, bool DEP>
hipError_t launch_variance_staged(bool staged, const rt_denoise_params& dp, const rt_denoise_variance_params& dv, hipStream_t st) {
    return staged ? launch_variance<NRM, DEP, true>(dp, dv, st) : launch_variance<NRM, DEP, false>(dp, dv, st);
}

}  // namespace

hipError_t rt_launch_denoise_pack_variance(const rt_denoise_params& dp, const rt_denoise_variance_params& dv, bool guide, hipStream_t st) {
    const size_t n = (size_t)dp.nx * dp.ny;
    const dim3 grid((unsigned)((n + RT_DENOISE_THREADS - 1) / RT_DENOISE_THREADS));
    if (guide) hipLaunchKernelGGL(rt_denoise_pack_variance_kernel<true>, grid, dim3(RT_DENOISE_THREADS), 0, st, dp, dv);
    else hipLaunchKernelGGL(rt_denoise_pack_variance_kernel<false>, grid, dim3(RT_DENOISE_THREADS), 0, st, dp, dv);
    return hipGetLastError();
}

hipError_t rt_launch_denoise_variance(bool normal_on, bool depth_on, bool staged, const rt_denoise_params& dp, const rt_denoise_variance_params& dv,
                                      hipStream_t st) {
    if (normal_on) return depth_on ? launch_variance_staged<true, true>(staged, dp, dv, st) : launch_variance_staged<true, false>(staged, dp, dv, st);
    return depth_on ? launch_variance_staged<false, true>(staged, dp, dv, st) : launch_variance_staged<false, false>(staged, dp, dv, st);
}
