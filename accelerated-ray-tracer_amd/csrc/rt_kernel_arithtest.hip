// rt_kernel_arithtest.hip -- rt_debug_arith_tests (include/rt_abi.h): the cheaper exact forms of rt_xorwow.h and
// rt_device_funcs.h (one-fma draws, the sign-folded loose_setup) compared inside the kernel, bit for bit, with the expressions
// they replace -- kept here in plain C++ as they were written first.  A test seam (tests/test_exact_arith.py), never on a
// frame's path.  Internal to librt_mi355x.so; launched by rt_abi.hip.
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

}  // namespace

hipError_t rt_launch_arith_tests(const rt_arith_test_params& ap, hipStream_t st) {
    if (ap.mode == RT_ARITH_UNIFORM || ap.mode == RT_ARITH_SIGNED) {
        const long long per_block = 256ll * RT_ARITH_WORDS_PER_THREAD;
        hipLaunchKernelGGL(rt_arith_draws_kernel, dim3((unsigned)((ap.n + per_block - 1) / per_block)), dim3(256), 0, st, ap);
    } else {
        hipLaunchKernelGGL(rt_arith_loose_kernel, dim3((unsigned)((ap.n + 255) / 256)), dim3(256), 0, st, ap);
    }
    return hipGetLastError();
}
