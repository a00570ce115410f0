"""The device's maths library against the oracle's, input by input.  Every GPU parity test of this suite asks
for equal float32 bits and so assumes that cr_log, cr_sin, cr_acos, cr_atan2, cr_pow and cr_pow5 of csrc/rt_device_funcs.h --
(float)fn((double)x) over the device library -- and the oracle's cr_*f -- the same over glibc -- are one function.  Neither
library is correctly rounded in double, so that is a measurable claim, not a given: the diagnostic entry rt_debug_math_tests
(include/rt_abi.h) runs the render path's own wrappers on chosen inputs, orc_math_sweep / orc_math_list run the oracle's, and
the two must agree with no tolerance:

  log      every float of (0, 1] -- a superset of what rt_uniform_from_word returns, the medium's only argument
  acos     every float of [-1, 1]; and a block of 2^20 floats beyond either end, where both sides must give NaN
  sin      every finite float, in six ranges: |x| < 1, 1 <= |x| <= 2^24 and |x| > 2^24, either sign
  pow      every float of [0, +inf] through apply_gamma at gamma 2.2; A SAMPLE at gamma 1.8, 2.0 and 2.4: 2^24 words 127 or 128
           apart over the same range
  pow5     every float of [0, 2]: the device's four double multiplies against the oracle's pow(x, 5.0)
  atan2    A SAMPLE, not a sweep (two inputs): 2^24 pairs (-p.z, p.x) of float32 unit vectors, the arguments sphere uv gives it;
           2^20 pairs with a component at +-0, subnormal or one ulp from +-1; the 6 x 6 grid of +-0, +-1, +- the smallest normal
  sqrtf, 1.0f / x      all 2^32 words against the host's IEEE results
  a / b    A SAMPLE: 2^24 pairs of random bit patterns, and quotients at the subnormal and the overflow edge
  a * b + c            2^20 triples with c = -fl(a * b) and an inexact product: the unfused value is +0, a fused one is not

Swept ranges are compared through one 64-bit digest per block of 2^20 words (tests/math_expect.py states it; the host file
shows that one flipped result bit changes it); a block that differs is run again in list form on both sides and every
disagreeing input is reported with both results and the correctly rounded value by mpmath.  Before that, per function, one
block's digest is checked on both sides against the NumPy digest of that side's list results.
"""
import json
import os
import time

import numpy as np
import pytest

import math_expect as M
from math_expect import F

pytestmark = pytest.mark.gpu
TINY = 0x00800000                                # the smallest normal


def report(domain, fn, operand, inputs, seconds, recs):
    """With RT_MATH_REPORT=<file> in the environment (how profiles/device_math_mi355x.jsonl was made): one line per domain, then
    one per disagreeing input.  Nothing is asserted on it."""
    if os.environ.get("RT_MATH_REPORT"):
        with open(os.environ["RT_MATH_REPORT"], "a") as f:
            head = {"domain": domain, "fn": M.NAMES[fn], "inputs": inputs, "disagreements_listed": len(recs), "seconds_device_oracle": seconds}
            if fn == M.POW:
                head["gamma"] = float(F(operand))
            f.write("\n".join(json.dumps(x) for x in [head] + recs) + "\n")


def swept(gpu, orc, fn, ranges, operand=0.0):
    """The ranges [(first word, count)] on both sides; prints the wall time; returns (inputs, blocks that differ, the records of
    the disagreeing inputs of the first 8 such blocks of each range)."""
    L = gpu.rt_lib()
    inputs, recs, blocks, t_dev, t_orc = 0, [], 0, 0.0, 0.0
    for first, count in ranges:
        n, r, td, to = M.compare_sweep(L, orc, fn, first, count, operand, max_blocks=8)
        inputs, recs, blocks, t_dev, t_orc = inputs + count, recs + r, blocks + n, t_dev + td, t_orc + to
    print(f"{M.NAMES[fn]}: {inputs} inputs, device {t_dev:.2f} s, oracle {t_orc:.2f} s, {blocks} blocks differ, {len(recs)} inputs listed")
    for r in recs[:64]:
        print("  ", r)
    report(" ".join(f"words 0x{first:08X} .. 0x{first + count - 1:08X}" for first, count in ranges), fn, operand, inputs, [round(t_dev, 3), round(t_orc, 3)], recs)
    return inputs, blocks, recs


def listed(gpu, orc, fn, a, b=None, c=None, domain="sample"):
    t0 = time.perf_counter()
    recs = M.compare_lists(gpu.rt_lib(), orc, fn, a, b, c)
    seconds = time.perf_counter() - t0
    print(f"{M.NAMES[fn]}: {len(a)} inputs in list form, {seconds:.2f} s, {len(recs)} disagree")
    for r in recs[:64]:
        print("  ", r)
    report(domain, fn, b[0] if fn == M.POW else 0.0, len(a), [round(seconds, 3)], recs[:1024])
    return recs


# ------------------------------------------------------------------ the digest itself, on both sides
@pytest.mark.parametrize("fn", [M.LOG, M.SIN, M.ACOS, M.POW, M.POW5, M.SQRT, M.RCP], ids=lambda fn: M.NAMES[fn])
def test_digest_is_the_digest_of_the_list(gpu, orc, fn):
    """One whole block and a short range off the 2^20 grid that spans three blocks: sweep digest == NumPy digest of the same
    side's list results.  A digest bug on either side cannot hide behind equal digests."""
    L = gpu.rt_lib()
    for first, count in [(0x3F000000, M.BLOCK), (M.ONE - M.BLOCK - 777, 2 * M.BLOCK + 999)]:
        got_dev, got_orc = M.dev_sweep(L, fn, first, count, 2.2), orc.math_sweep(fn, first, count, 2.2)
        for k, w0 in enumerate(range(first, first + count, M.BLOCK)):
            n = min(M.BLOCK, first + count - w0)
            a = M.words_as_floats(w0, n)
            b = np.full(n, 2.2, F) if fn == M.POW else None
            assert got_dev[k] == M.digest(a.view(np.uint32), M.dev_list(L, fn, a, b)), (M.NAMES[fn], "device", hex(w0), n)
            assert got_orc[k] == M.digest(a.view(np.uint32), orc.math_list(fn, a, b)), (M.NAMES[fn], "oracle", hex(w0), n)


# ------------------------------------------------------------------ exhaustive
def test_log_every_float_of_0_to_1(gpu, orc):
    _, blocks, recs = swept(gpu, orc, M.LOG, [(1, M.ONE)])                                # the smallest subnormal .. 1.0
    assert blocks == 0, recs[:16]


@pytest.mark.parametrize("sign", [0, M.NEG], ids=["plus", "minus"])
def test_acos_every_float_of_its_domain(gpu, orc, sign):
    _, blocks, recs = swept(gpu, orc, M.ACOS, [(sign, M.ONE + 1)])                        # +-0 .. +-1.0
    assert blocks == 0, recs[:16]


@pytest.mark.parametrize("sign", [0, M.NEG], ids=["plus", "minus"])
def test_acos_beyond_its_domain_is_nan_on_both_sides(gpu, orc, sign):
    first = sign + M.ONE + 1
    a = M.words_as_floats(first, M.BLOCK)
    all_nan = M.digest(a.view(np.uint32), np.full(M.BLOCK, np.nan, F))
    assert M.dev_sweep(gpu.rt_lib(), M.ACOS, first, M.BLOCK)[0] == all_nan == orc.math_sweep(M.ACOS, first, M.BLOCK)[0]


# |x| < 1, 1 <= |x| <= 2^24, |x| > 2^24: (first word, count) without the sign
SIN_RANGES = {"below_1": (0, M.ONE), "1_to_2p24": (M.ONE, M.TWO24 + 1 - M.ONE), "above_2p24": (M.TWO24 + 1, M.INF - M.TWO24 - 1)}


@pytest.mark.parametrize("sign", [0, M.NEG], ids=["plus", "minus"])
@pytest.mark.parametrize("span", list(SIN_RANGES))
def test_sin_every_finite_float(gpu, orc, span, sign):
    first, count = SIN_RANGES[span]
    _, blocks, recs = swept(gpu, orc, M.SIN, [(sign + first, count)])
    assert blocks == 0, recs[:16]


@pytest.mark.parametrize("half", [0, 1])
def test_pow_every_float_of_0_to_inf_at_gamma_2_2(gpu, orc, half):
    cut = 0x3F000000                                                                      # 0.5: about half the glibc time either side
    _, blocks, recs = swept(gpu, orc, M.POW, [(0, cut)] if half == 0 else [(cut, M.INF + 1 - cut)], 2.2)
    assert blocks == 0, recs[:16]


@pytest.mark.parametrize("gamma", [1.8, 2.0, 2.4])
def test_pow_strided_at_other_gammas(gpu, orc, gamma):
    words = (np.arange(1 << 24, dtype=np.uint64) * np.uint64(M.INF)) // np.uint64((1 << 24) - 1)   # +0 .. +inf, 127 or 128 words apart
    a = words.astype(np.uint32).view(F)
    assert a[0] == 0 and np.isposinf(a[-1]) and not np.isnan(a).any()
    assert listed(gpu, orc, M.POW, a, np.full(len(a), gamma, F), domain="2^24 words spread evenly over +0 .. +inf") == []


def test_pow5_every_float_of_0_to_2(gpu, orc):
    _, blocks, recs = swept(gpu, orc, M.POW5, [(0, M.TWO + 1)])
    assert blocks == 0, recs[:16]


@pytest.mark.parametrize("fn", [M.SQRT, M.RCP], ids=lambda fn: M.NAMES[fn])
def test_sqrt_and_reciprocal_are_ieee_on_all_words(gpu, orc, fn):
    _, blocks, recs = swept(gpu, orc, fn, [(0, 1 << 32)])
    assert blocks == 0, recs[:16]


# ------------------------------------------------------------------ sampled
def unit_vectors(rng, n):
    """float32 unit vectors as unit_vector (rt_device_funcs.h) leaves them: v / sqrtf(dot(v, v)), each step in float32."""
    v = rng.standard_normal((n, 3), dtype=F)
    ln = np.sqrt((v[:, 2] * v[:, 2] + (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(F)).astype(F)).astype(F)
    return (v / ln[:, None]).astype(F)


def test_atan2_on_unit_vectors_sampled(gpu, orc):
    """A sample: 2^24 of the 2^64 pairs.  (-p.z, p.x) as get_sphere_uv passes them."""
    p = unit_vectors(np.random.default_rng(20261021), 1 << 24)
    assert listed(gpu, orc, M.ATAN2, np.ascontiguousarray(-p[:, 2]), np.ascontiguousarray(p[:, 0]), domain="2^24 pairs (-p.z, p.x) of unit vectors") == []


def test_atan2_at_the_edges_sampled(gpu, orc):
    """A sample: 2^20 pairs, one component +-0, subnormal or one ulp from +-1, the other a unit vector's or a random pattern."""
    rng = np.random.default_rng(20261022)
    n = 1 << 20
    special = np.concatenate([np.array([0, 1, 0x007FFFFF, M.ONE - 1, M.ONE, M.ONE + 1], np.uint32), rng.integers(1, TINY, 58).astype(np.uint32)])
    s = special[rng.integers(0, len(special), n)] | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))
    other = np.where(rng.random(n) < 0.5, unit_vectors(rng, n)[:, 0].view(np.uint32), rng.integers(0, M.INF, n).astype(np.uint32)
                     | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))).astype(np.uint32)
    first = rng.random(n) < 0.5
    a, b = np.where(first, s, other).view(F), np.where(first, other, s).view(F)
    assert listed(gpu, orc, M.ATAN2, a, b, domain="2^20 pairs with a component +-0, subnormal or one ulp from +-1") == []


def test_atan2_on_the_grid_of_zeros_ones_and_tiny(gpu, orc):
    g = np.array([0, M.NEG, M.ONE, M.ONE | M.NEG, TINY, TINY | M.NEG], np.uint32).view(F)
    a, b = (np.ascontiguousarray(x.reshape(-1)) for x in np.meshgrid(g, g, indexing="ij"))
    dev, ref = M.dev_list(gpu.rt_lib(), M.ATAN2, a, b), orc.math_list(M.ATAN2, a, b)
    ieee = np.arctan2(a.astype(np.float64), b.astype(np.float64)).astype(F)              # the signs of zero and pi included
    print("atan2 grid:", [(float(x), float(y), float(d)) for x, y, d in zip(a, b, dev)])
    assert np.array_equal(dev.view(np.uint32), ref.view(np.uint32)) and np.array_equal(ref.view(np.uint32), ieee.view(np.uint32))


def test_division_sampled(gpu, orc):
    """A sample: 2^24 - 2^16 pairs of random bit patterns (NaN, inf, zeros and subnormals among them), and 2^16 quotients that
    land within a few ulp of the smallest normal, the smallest subnormal and FLT_MAX; the host's IEEE division is the reference."""
    rng = np.random.default_rng(20261023)
    n, ne = (1 << 24) - (1 << 16), 1 << 16
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(F)
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(F)
    target = np.array([TINY, 1, 2, 0x7F7FFFFF, 0x007FFFFF, TINY + 1], np.uint32).view(F)[rng.integers(0, 6, ne)]
    eb = (rng.integers(M.ONE - (20 << 23), M.ONE + (20 << 23), ne).astype(np.uint32) | (rng.integers(0, 2, ne).astype(np.uint32) << np.uint32(31))).view(F)
    with np.errstate(over="ignore", under="ignore"):
        ea = (target.astype(np.float64) * eb.astype(np.float64) * rng.choice([0.5, 0.75, 1.0, 1.0, 1.5, 2.0], ne)).astype(F)
    a, b = np.concatenate([a, ea]), np.concatenate([b, eb])
    assert listed(gpu, orc, M.DIV, a, b, domain="2^24 pairs: random bit patterns, quotients at the subnormal and overflow edges") == []
    with np.errstate(all="ignore"):
        host = (a / b).astype(F)
    assert np.array_equal(M.canonical_bits(orc.math_list(M.DIV, a, b)), M.canonical_bits(host))


def test_product_and_sum_are_not_fused(gpu, orc):
    """a * b + c with c = -fl(a * b) on 2^20 triples whose product is inexact in float32: rounded as written, the value is +0;
    a fused multiply-add would give a * b - fl(a * b), which is not zero.  The device must give the unfused value."""
    rng = np.random.default_rng(20261024)
    n = 1 << 20
    a = rng.integers(M.ONE, M.TWO, 2 * n).astype(np.uint32).view(F) * F(2.0) ** rng.integers(-20, 20, 2 * n).astype(F)
    b = rng.integers(M.ONE, M.TWO, 2 * n).astype(np.uint32).view(F) * F(2.0) ** rng.integers(-20, 20, 2 * n).astype(F)
    exact = a.astype(np.float64) * b.astype(np.float64)                                  # 48 bits: exact in float64
    keep = np.flatnonzero(exact.astype(F).astype(np.float64) != exact)[:n]
    assert len(keep) == n
    a, b = np.ascontiguousarray(a[keep]), np.ascontiguousarray(b[keep])
    c = -(a * b).astype(F)
    fused = (exact[keep] + c.astype(np.float64)).astype(F)
    assert (fused != 0).all()
    assert listed(gpu, orc, M.MULADD, a, b, c, domain="2^20 triples with c = -fl(a * b), inexact products") == []
    dev = M.dev_list(gpu.rt_lib(), M.MULADD, a, b, c)
    assert (dev.view(np.uint32) == 0).all(), int((dev.view(np.uint32) != 0).sum())     # +0 everywhere: the unfused value
