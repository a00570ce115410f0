// rt_kernel_arithtest.hip -- rt_debug_arith_tests (include/rt_abi.h): the cheaper exact forms of rt_xorwow.h and
// rt_device_funcs.h (one-fma draws, the sign-folded loose_setup) compared inside the kernel, bit for bit, with the expressions
// they replace -- kept here in plain C++ as they were written first.  A test seam (tests/test_exact_arith.py), never on a
// frame's path.  Internal to librt_mi355x.so; launched by rt_abi.hip.
// Also rt_debug_math_tests: the transcendental wrappers of rt_device_funcs.h (cr_log, cr_sin, cr_acos, cr_atan2, cr_pow through
// apply_gamma, cr_pow5) and the contract's plain operations (sqrtf, /, an unfused a * b + c) on caller-chosen inputs, for
// tests/test_device_math.py to compare with the oracle's library input by input.  The functions called are the render path's.
#define RT_DRAW_ONE_FMA 1   // rt_xorwow.h: the form under test
#include "rt_device_funcs.h"

namespace {

// the forms replaced
DEV float old_uniform(uint32_t x) { return (float)x * 2.3283064e-10f + (2.3283064e-10f / 2.0f); }
DEV float old_signed(uint32_t x) { return 2.0f * old_uniform(x) - 1.0f; }
DEV LooseRay old_loose_setup(const f3 inv, const f3 o, const float* bound) {
    const float k = 9.5367431640625e-07f;   // 2^-20
    const float ex = k * (fabsf(inv.x) * (fabsf(o.x) + bound[0])), ey = k * (fabsf(inv.y) * (fabsf(o.y) + bound[1])), ez = k * (fabsf(inv.z) * (fabsf(o.z) + bound[2]));
    const float cx = -(o.x * inv.x), cy = -(o.y * inv.y), cz = -(o.z * inv.z);
    LooseRay r;
    r.clo = mk3(inv.x < 0.0f ? cx + ex : cx - ex, inv.y < 0.0f ? cy + ey : cy - ey, inv.z < 0.0f ? cz + ez : cz - ez);
    r.chi = mk3(inv.x < 0.0f ? cx - ex : cx + ex, inv.y < 0.0f ? cy - ey : cy + ey, inv.z < 0.0f ? cz - ez : cz + ez);
    return r;
}

DEV bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }
DEV bool same_bits(f3 a, f3 b) { return same_bits(a.x, b.x) && same_bits(a.y, b.y) && same_bits(a.z, b.z); }

// the two draw modes: words [0, n), RT_ARITH_WORDS_PER_THREAD consecutive words a thread
__global__ void __launch_bounds__(256) rt_arith_draws_kernel(rt_arith_test_params ap) {
    const unsigned long long first = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * RT_ARITH_WORDS_PER_THREAD;
    unsigned int bad = 0u;
    unsigned long long first_bad = ~0ull;
    for (unsigned int k = 0; k < RT_ARITH_WORDS_PER_THREAD; ++k) {
        const unsigned long long w = first + k;
        if (w >= (unsigned long long)ap.n) break;
        const uint32_t x = (uint32_t)w;
        const bool equal = ap.mode == RT_ARITH_UNIFORM ? same_bits(rt_uniform_from_word(x), old_uniform(x)) : same_bits(rt_signed_from_word(x), old_signed(x));
        if (!equal) { ++bad; if (first_bad == ~0ull) first_bad = w; }
    }
    if (bad) { atomicAdd(ap.out, (unsigned long long)bad); atomicMin(ap.out + 1, first_bad); }
}

// RT_ARITH_LOOSE: one ray per thread, its box-test terms as stage F and the trip of the main kernel set them up
__global__ void __launch_bounds__(256) rt_arith_loose_kernel(rt_arith_test_params ap) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ap.n) return;
    const f3 o = ld3(ap.a + 3 * i), d = ld3(ap.b + 3 * i);
    const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    const bool finite_inv = inv_is_finite(inv) && loose_ok(inv, o, ap.bound);   // the rays the walk loop admits
    const LooseRay now = loose_setup(inv, o, ap.bound), then = old_loose_setup(inv, o, ap.bound);
    if (ap.path) ap.path[i] = finite_inv ? 1 : 0;
    if (!finite_inv) return;
    atomicAdd(ap.out + 2, 1ull);
    if (!(same_bits(now.clo, then.clo) && same_bits(now.chi, then.chi))) { atomicAdd(ap.out, 1ull); atomicMin(ap.out + 1, (unsigned long long)i); }
}

// ------------------------------------------------------------------ rt_debug_math_tests
DEV float math_eval(int fn, float a, float b, float c) {
    switch (fn) {
    case RT_MATH_LOG: return cr_log(a);
    case RT_MATH_SIN: return cr_sin(a);
    case RT_MATH_ACOS: return cr_acos(a);
    case RT_MATH_ATAN2: return cr_atan2(a, b);
    case RT_MATH_POW: return apply_gamma(a, b);
    case RT_MATH_POW5: return cr_pow5(a);
    case RT_MATH_SQRT: return sqrtf(a);
    case RT_MATH_RCP: return 1.0f / a;
    case RT_MATH_DIV: return a / b;
    default: return a * b + c;   // RT_MATH_MULADD: as written; this unit is built with -ffp-contract=off like every other
    }
}

// include/rt_abi.h states it: the finaliser of splitmix64 over (word, result bits), every NaN as 0x7FC00000
DEV unsigned long long mix64(uint32_t w, float r) {
    const uint32_t bits = r != r ? 0x7FC00000u : __float_as_uint(r);
    unsigned long long z = ((unsigned long long)w << 32) | bits;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// RT_MATH_SWEEP: a workgroup takes RT_MATH_WORDS_PER_GROUP consecutive words -- all of one 2^20 block, 2^20 being a multiple --
// sums their mix64 through LDS and adds the sum into the block's digest (a sum modulo 2^64: any order)
__global__ void __launch_bounds__(256) rt_math_sweep_kernel(rt_math_test_params mp) {
    __shared__ unsigned long long part[256];
    const unsigned long long base = (unsigned long long)blockIdx.x * RT_MATH_WORDS_PER_GROUP;
    unsigned long long sum = 0ull;
    for (unsigned int k = threadIdx.x; k < RT_MATH_WORDS_PER_GROUP; k += 256u) {
        const unsigned long long i = base + k;
        if (i >= (unsigned long long)mp.count) break;
        const uint32_t w = mp.first + (uint32_t)i;   // first + count <= 2^32: no wrap
        sum += mix64(w, math_eval(mp.fn, __uint_as_float(w), mp.operand, 0.0f));
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (unsigned int h = 128u; h > 0u; h >>= 1) {
        if (threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0u) atomicAdd(mp.digests + (base >> 20), part[0]);
}

// RT_MATH_LIST: one element per thread
__global__ void __launch_bounds__(256) rt_math_list_kernel(rt_math_test_params mp) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mp.count) return;
    mp.out[i] = math_eval(mp.fn, mp.a[i], mp.b ? mp.b[i] : 0.0f, mp.c ? mp.c[i] : 0.0f);
}

}  // namespace

hipError_t rt_launch_math_tests(const rt_math_test_params& mp, hipStream_t st) {
    if (mp.form == RT_MATH_SWEEP)
        hipLaunchKernelGGL(rt_math_sweep_kernel, dim3((unsigned)((mp.count + RT_MATH_WORDS_PER_GROUP - 1) / RT_MATH_WORDS_PER_GROUP)), dim3(256), 0, st, mp);
    else
        hipLaunchKernelGGL(rt_math_list_kernel, dim3((unsigned)((mp.count + 255) / 256)), dim3(256), 0, st, mp);
    return hipGetLastError();
}

hipError_t rt_launch_arith_tests(const rt_arith_test_params& ap, hipStream_t st) {
    if (ap.mode == RT_ARITH_UNIFORM || ap.mode == RT_ARITH_SIGNED) {
        const long long per_block = 256ll * RT_ARITH_WORDS_PER_THREAD;
        hipLaunchKernelGGL(rt_arith_draws_kernel, dim3((unsigned)((ap.n + per_block - 1) / per_block)), dim3(256), 0, st, ap);
    } else {
        hipLaunchKernelGGL(rt_arith_loose_kernel, dim3((unsigned)((ap.n + 255) / 256)), dim3(256), 0, st, ap);
    }
    return hipGetLastError();
}
