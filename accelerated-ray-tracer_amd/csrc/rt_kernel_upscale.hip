// rt_kernel_upscale.hip -- rt_upscale: the guided (joint bilateral) upscaler of include/rt_abi.h ("upscaler"), gfx950.
//
// One kernel, the denoiser's workgroup: 256 threads = four waves on 8x8 output pixels each = a 16x16 tile of the output, one
// output pixel per lane in registers.  A pixel reads its own guides (planar, once) and nine coarse taps; a coarse pixel is two
// 16-byte records, colour (x.rgb, the demodulating divisions done) and guide (N.xyz, Z; zeros where a factor is off).
// The tile, the records' contents, the two factors and the remodulation are the denoiser's definitions (rt_filter.h).
// Specialised on which of the two factors are on and on how the taps are fetched:
//   staged  the window of coarse pixels the tile's taps reach -- at most 11 x 11 (rt_device.h) -- is prepared once per
//           workgroup into LDS, and the nine taps of every pixel are LDS reads;
//   direct  every tap is read from the planar coarse images through L1/L2 and prepared where it is used.
// Which one a call gets is the host's choice (rt_abi.hip, option "upscale_lds"); preparing a record is the
// same divisions on the same operands in both, and the taps run through the same statements in the same order, so the choice
// changes no bit.
//
// Bounds: a tap outside the coarse image is skipped by an index test before any address is formed; the staging loop loads only
// the records inside the coarse image, and a tap that passes the index test lies inside the staged window by construction
// (its column is within one of a column I = i / f of the tile, and the window starts at x0 / f - 1), so no slot is read that
// was not written.  No address depends on pixel data.
#include "rt_device.h"
#include "rt_filter.h"
#include "rt_launch.h"

namespace {

using namespace rt_filter;
constexpr int WIN = RT_UPSCALE_WINDOW;

// "Prepare" of the contract for coarse pixel q: x(q) and, where a factor is on, its guides
// (the block by value and the guides fetched first: with the direct taps this order and form run 4 % faster than the colour
// first through a reference; no operation depends on the order; profiles/filter_shared_mi355x.jsonl)
template <bool NRM, bool DEP>
__device__ __forceinline__ void coarse_record(const rt_upscale_params up, size_t q, float4& x, float4& g) {
    g = guide_record(NRM, DEP, up.normal_lo, up.depth_lo, q);
    const float3 c = demodulated(up.color_lo, up.albedo_lo, up.demodulate, q);
    x = make_float4(c.x, c.y, c.z, 0.f);
}

// "Position" of the contract: B[-1], B[0], B[+1] for the offset r = i - I f of an output coordinate in its coarse pixel
__device__ __forceinline__ void spline_weights(unsigned r, int f, float B[3]) {
    const float c = (float)(2 * r + 1) / (float)(2 * f) - 0.5f;
    const float a = 0.5f - c, b = 0.5f + c;
    B[0] = 0.5f * (a * a);
    B[1] = 0.75f - c * c;
    B[2] = 0.5f * (b * b);
}

template <bool NRM, bool DEP, bool STAGED>
__global__ __launch_bounds__(RT_DENOISE_THREADS) void rt_upscale_kernel(rt_upscale_params up) {
    __shared__ float4 lds[STAGED ? 2 * WIN * WIN : 1];
    constexpr bool GUIDE = NRM || DEP;
    const int tid = threadIdx.x;
    const int nx = up.nx, ny = up.ny, lx = up.lx, ly = up.ly, f = up.factor;
    const tile_pixel tile = tile_mapping(up.tiles_x);
    const unsigned i = tile.i, j = tile.j;

    const unsigned ox = (unsigned)tile.x0 / (unsigned)f - 1u, oy = (unsigned)tile.y0 / (unsigned)f - 1u;   // coarse coordinates of LDS slot (0, 0)
    const float4* lc = lds;
    const float4* lg = lds + WIN * WIN;
    if (STAGED) {
        if (tid < WIN * WIN) {
            const int wy = tid / WIN, wx = tid - wy * WIN;
            const unsigned gx = ox + wx, gy = oy + wy;
            if (gx < (unsigned)lx && gy < (unsigned)ly) {
                float4 x, g;
                coarse_record<NRM, DEP>(up, (size_t)gy * lx + gx, x, g);
                lds[tid] = x;
                if (GUIDE) lds[WIN * WIN + tid] = g;
            }
        }
        __syncthreads();
    }
    if (i >= (unsigned)nx || j >= (unsigned)ny) return;

    const size_t p = (size_t)j * nx + i;
    const float4 gp = guide_record(NRM, DEP, up.normal, up.depth, p);

    const unsigned I = i / (unsigned)f, J = j / (unsigned)f;
    float Bx[3], By[3];
    spline_weights(i - I * (unsigned)f, f, Bx);
    spline_weights(j - J * (unsigned)f, f, By);

    float W0 = 0.f, S0r = 0.f, S0g = 0.f, S0b = 0.f;
    float W = 0.f, Sr = 0.f, Sg = 0.f, Sb = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const unsigned qy = J + (unsigned)dy;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const unsigned qx = I + (unsigned)dx;
            if (qx >= (unsigned)lx || qy >= (unsigned)ly) continue;
            float4 xq, gq = make_float4(0.f, 0.f, 0.f, 0.f);
            if (STAGED) {
                const int c = (int)(qy - oy) * WIN + (int)(qx - ox);
                xq = lc[c];
                if (GUIDE) gq = lg[c];
            } else {
                coarse_record<NRM, DEP>(up, (size_t)qy * lx + qx, xq, gq);
            }
            const float g = By[dy + 1] * Bx[dx + 1];
            float w = g;
            if (NRM) w = w * normal_factor(gp, gq, up.normal_sharpness);
            if (DEP) w = w * depth_factor(gp, gq, up.sigma_depth);
            W0 = W0 + g;
            S0r = S0r + g * xq.x;
            S0g = S0g + g * xq.y;
            S0b = S0b + g * xq.z;
            W = W + w;
            Sr = Sr + w * xq.x;
            Sg = Sg + w * xq.y;
            Sb = Sb + w * xq.z;
        }
    }
    // "Choose": the guided sums where enough of the spline's weight survived the factors, else the plain spline
    const bool guided = W >= up.min_weight * W0 && W > 0.f;
    const float den = guided ? W : W0;
    float r = (guided ? Sr : S0r) / den, g = (guided ? Sg : S0g) / den, b = (guided ? Sb : S0b) / den;
    remodulate(up.albedo, up.demodulate, p, r, g, b);
    up.out[3 * p] = r;
    up.out[3 * p + 1] = g;
    up.out[3 * p + 2] = b;
    if (up.weight_out) up.weight_out[p] = W / W0;
}

template <bool NRM, bool DEP, bool STAGED>
hipError_t launch(const rt_upscale_params& up, hipStream_t st) {
    const unsigned tiles_y = ((unsigned)up.ny + TILE - 1) / TILE;
    return rt_launch_kernel(rt_upscale_kernel<NRM, DEP, STAGED>, dim3(RT_DENOISE_THREADS), dim3((unsigned)up.tiles_x * tiles_y), 0, st, up);
}

template <bool NRM, bool DEP>
hipError_t launch_staged(bool staged, const rt_upscale_params& up, hipStream_t st) {
    return staged ? launch<NRM, DEP, true>(up, st) : launch<NRM, DEP, false>(up, st);
}

}  // namespace

hipError_t rt_launch_upscale(bool normal_on, bool depth_on, bool staged, const rt_upscale_params& up, hipStream_t st) {
    if (normal_on) return depth_on ? launch_staged<true, true>(staged, up, st) : launch_staged<true, false>(staged, up, st);
    return depth_on ? launch_staged<false, true>(staged, up, st) : launch_staged<false, false>(staged, up, st);
}
