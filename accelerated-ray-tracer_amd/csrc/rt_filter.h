// rt_filter.h -- what the image-space filters share on the device (rt_kernel_denoise.hip, rt_kernel_upscale.hip): the workgroup's
// tile, a pixel's guide record and demodulated colour, and the two guide factors of a tap.  Internal, device-only.
//
// The filters' results are bit-exact against host restatements (tests/denoise_expect.py, tests/upscale_expect.py), so every
// function here is the contract's statements in the contract's order: one rounding per written operation, nothing reassociated
// (the library is built with -ffp-contract=off).  All of it inlines; flags that are template parameters of a kernel arrive as
// constants and fold.
#pragma once
#include "rt_device.h"

namespace rt_filter {

constexpr int TILE = RT_DENOISE_TILE;
constexpr float ALBEDO_FLOOR = 0.0009765625f;   // 2^-10

// A workgroup of RT_DENOISE_THREADS on one 16x16 tile at (x0, y0), row bands of `tiles_x` tiles: a wave on one 8x8 tile, as in
// the other kernels, one pixel (i, j) per lane.
// (coordinates are unsigned: one below 0 or past 2^31 - 1 wraps and compares as out of the image)
struct tile_pixel { int x0, y0; unsigned i, j; };
__device__ __forceinline__ tile_pixel tile_mapping(int tiles_x) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int by = (int)(blockIdx.x / (unsigned)tiles_x), bx = (int)(blockIdx.x - (unsigned)by * (unsigned)tiles_x);
    tile_pixel t;
    t.x0 = bx * TILE; t.y0 = by * TILE;
    t.i = (unsigned)t.x0 + (wave & 1) * 8 + (lane & 7); t.j = (unsigned)t.y0 + (wave >> 1) * 8 + (lane >> 3);
    return t;
}

// the guide record of pixel p: N.xyz and Z, zeros where a guide is off
__device__ __forceinline__ float4 guide_record(bool normal_on, bool depth_on, const float* normal, const float* depth, size_t p) {
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (normal_on) { q.x = normal[3 * p]; q.y = normal[3 * p + 1]; q.z = normal[3 * p + 2]; }
    if (depth_on) q.w = depth[p];
    return q;
}

// the colour of pixel p, divided by its floored albedo when `demodulate`; and the way back
__device__ __forceinline__ float3 demodulated(const float* color, const float* albedo, int demodulate, size_t p) {
    float r = color[3 * p], g = color[3 * p + 1], b = color[3 * p + 2];
    if (demodulate) {
        r = r / fmaxf(albedo[3 * p], ALBEDO_FLOOR);
        g = g / fmaxf(albedo[3 * p + 1], ALBEDO_FLOOR);
        b = b / fmaxf(albedo[3 * p + 2], ALBEDO_FLOOR);
    }
    return make_float3(r, g, b);
}
__device__ __forceinline__ void remodulate(const float* albedo, int demodulate, size_t p, float& r, float& g, float& b) {
    if (demodulate) {
        r = r * fmaxf(albedo[3 * p], ALBEDO_FLOOR);
        g = g * fmaxf(albedo[3 * p + 1], ALBEDO_FLOOR);
        b = b * fmaxf(albedo[3 * p + 2], ALBEDO_FLOOR);
    }
}

// t of the contract: carries the variance of r + g + b over to the demodulated image and back
__device__ __forceinline__ float variance_scale(const float* albedo, size_t q) {
    const float ar = fmaxf(albedo[3 * q], ALBEDO_FLOOR), ag = fmaxf(albedo[3 * q + 1], ALBEDO_FLOOR), ab = fmaxf(albedo[3 * q + 2], ALBEDO_FLOOR);
    return 3.0f / ((ar + ag) + ab);
}

// the factors of a tap between guide records gp and gq: max(N_p . N_q, 0)^(2^m), and (1 - |Z_p - Z_q| / (sigma max(Z) + 1e-20))_+^2
__device__ __forceinline__ float normal_factor(const float4& gp, const float4& gq, int sharpness) {
    float d = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
    d = fmaxf(d, 0.f);
    for (int m = 0; m < sharpness; ++m) d = d * d;
    return d;
}
__device__ __forceinline__ float depth_factor(const float4& gp, const float4& gq, float sigma_depth) {
    const float den = sigma_depth * fmaxf(gp.w, gq.w) + 1e-20f;
    const float r = fabsf(gp.w - gq.w) / den;
    const float t = fmaxf(1.f - r, 0.f);
    return t * t;
}

}  // namespace rt_filter
