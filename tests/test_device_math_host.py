"""The CPU half of the maths-library comparison (the GPU half is tests/test_device_math.py).  The suite's zero
tolerance rests on the device's and the oracle's transcendentals being the same float32 function; the oracle's are
(float)fn((double)x) over glibc.  Here, without a GPU:

  digest     the oracle's sweep digests (orc_math_sweep) equal a NumPy restatement of the digest computed from its list results
             (orc_math_list), per function that has a sweep form (those of one input, and pow) on a few blocks -- whole, short,
             and off the 2^20 grid; and one flipped result bit in a list changes the NumPy digest, so equality of digests is as
             strict as equality of every result
  pow5       Schlick's fifth power: the product form the device uses (four double multiplies, rounded once) equals the oracle's
             pow(x, 5.0) rounded once on EVERY float of [0, 2]
  mpmath     on a fixed sample of 4096 inputs per function -- 0.5, 1, the powers of two and the floats one ulp either side, then
             random bit patterns -- the oracle's result is the correctly rounded float32 of the true value (256 bits)
  arguments  rt_debug_math_tests refuses bad arguments before it touches the device
"""
import time

import numpy as np
import pytest

import math_expect as M
from math_expect import F

ONE_INPUT = [M.LOG, M.SIN, M.ACOS, M.POW5, M.SQRT, M.RCP, M.POW5_PRODUCT]
# (first word, count): a block of (0, 1), a short one, one that straddles 1.0 off the 2^20 grid, two and a bit of large negatives
RANGES = [(0x3F000000, M.BLOCK), (0x00000001, 777), (M.ONE - 12345, M.BLOCK + 99), (0xC0000000 - 5, 2 * M.BLOCK + 7)]


def numpy_digests(orc, fn, first, count, operand=0.0):
    out = []
    for w0 in range(first, first + count, M.BLOCK):
        n = min(M.BLOCK, first + count - w0)
        a = M.words_as_floats(w0, n)
        r = orc.math_list(fn, a, np.full(n, operand, F) if fn == M.POW else None)
        out.append(M.digest(a.view(np.uint32), r))
    return np.array(out, np.uint64)


@pytest.mark.parametrize("fn", ONE_INPUT + [M.POW], ids=lambda fn: M.NAMES[fn])
def test_sweep_digest_is_the_digest_of_the_list(orc, fn):
    for first, count in RANGES:
        got = orc.math_sweep(fn, first, count, 2.2, threads=3)
        assert np.array_equal(got, numpy_digests(orc, fn, first, count, 2.2)), (M.NAMES[fn], hex(first), count)
        assert np.array_equal(got, orc.math_sweep(fn, first, count, 2.2, threads=1))     # however the work is split


def test_nan_results_count_as_one_pattern(orc):
    a = M.words_as_floats(0xBF800001, 4096)                                               # below -1: acos and log give NaN
    for fn in (M.ACOS, M.LOG):
        r = orc.math_list(fn, a)
        assert np.isnan(r).all()
        want = M.mix64(a.view(np.uint32), np.full(len(a), 0x7FC00000, np.uint32)).sum(dtype=np.uint64)
        assert orc.math_sweep(fn, 0xBF800001, 4096)[0] == want == M.digest(a.view(np.uint32), -r)   # -NaN: another sign, same digest


def test_one_flipped_result_bit_changes_the_digest(orc):
    """What makes digest equality a test of every result: a one-ulp change of any single result moves the block's digest."""
    a = M.words_as_floats(0x3F000000, M.BLOCK)
    r = orc.math_list(M.LOG, a)
    base = M.digest(a.view(np.uint32), r)
    rng = np.random.default_rng(7)
    for i in [0, M.BLOCK - 1] + list(rng.integers(0, M.BLOCK, 30)):
        bits = r.view(np.uint32).copy()
        bits[i] ^= np.uint32(1)
        assert M.digest(a.view(np.uint32), bits.view(F)) != base, i
    swapped = r.copy()
    swapped[[0, 1]] = r[[1, 0]]                                                            # the word is mixed in: results cannot trade places
    assert M.digest(a.view(np.uint32), swapped) != base


def test_pow5_product_form_is_pow_on_every_float_of_0_to_2(orc):
    t0 = time.perf_counter()
    count = M.TWO + 1                                                                      # +0 .. 2.0, every float
    product, libm = orc.math_sweep(M.POW5_PRODUCT, 0, count), orc.math_sweep(M.POW5, 0, count)
    print(f"pow5: {count} inputs, {len(product)} blocks, {time.perf_counter() - t0:.2f} s")
    differ = np.flatnonzero(product != libm)
    detail = []
    for k in differ[:4]:
        a = M.words_as_floats(int(k) * M.BLOCK, min(M.BLOCK, count - int(k) * M.BLOCK))
        p, q = orc.math_list(M.POW5_PRODUCT, a), orc.math_list(M.POW5, a)
        bad = np.flatnonzero(p.view(np.uint32) != q.view(np.uint32))
        detail += [(hex(a.view(np.uint32)[i]), hex(p.view(np.uint32)[i]), hex(q.view(np.uint32)[i])) for i in bad[:8]]
    assert len(differ) == 0, (len(differ), detail)


@pytest.mark.parametrize("fn", [M.LOG, M.SIN, M.ACOS, M.ATAN2, M.POW, M.POW5, M.POW5_PRODUCT], ids=lambda fn: M.NAMES[fn])
def test_oracle_is_correctly_rounded_on_the_sample(orc, fn):
    a, b = M.sample(fn)
    t0 = time.perf_counter()
    got = orc.math_list(fn, a, b).view(np.uint32)
    want = M.correct_bits(fn, a, b)
    print(f"{M.NAMES[fn]}: {len(a)} inputs against mpmath at {M.PREC} bits, {time.perf_counter() - t0:.2f} s")
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(hex(a.view(np.uint32)[i]), None if b is None else float(b[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]


def test_round_bits_rounds_to_nearest_even():
    """The arbiter's own rounding, on values whose float32 is known: ties, subnormals, the overflow threshold."""
    import mpmath
    with mpmath.workprec(M.PREC):
        two = mpmath.mpf(2)
        cases = [(mpmath.mpf(1), 0x3F800000), (1 + two ** -24, 0x3F800000), (1 + 3 * two ** -24, 0x3F800002), (1 + two ** -24 + two ** -200, 0x3F800001),
                 (-(1 + two ** -23), 0xBF800001), (two ** -149, 1), (two ** -150, 0), (3 * two ** -150, 2), (two ** -126 - two ** -150, 0x00800000),
                 (two ** 128 - two ** 103, 0x7F800000), (two ** 128 - two ** 103 - two ** 50, 0x7F7FFFFF), (mpmath.mpf(31) ** 5, int(F(31 ** 5).view(np.uint32)))]
        for v, bits in cases:
            assert M.round_bits(v) == bits, (v, hex(M.round_bits(v)), hex(bits))
    assert 31 ** 5 % 2 == 1 and 31 ** 5 > 1 << 24                                         # an exact tie of pow5: 25 bits, odd


# (loads the render library: after the oracle's tests on purpose, as tests/test_exact_arith.py's last test explains)
def test_argument_checks_run_before_the_device(art):
    """An unknown form or function, a sweep of a two-input function, null or surplus pointers, a count out of range and a bad
    gamma are RT_ERR_INVALID with a detail string; what passes the checks gets as far as the device and no further."""
    L = art.rt_lib()
    v = np.ones(4, F)
    dig = np.zeros(4, np.uint64)
    A, D = v.ctypes.data, dig.ctypes.data
    S, T = M.SWEEP, M.LIST
    bad = [[2, M.LOG, 0, 1, 0.0, None, None, None, None, D], [-1, M.LOG, 0, 1, 0.0, None, None, None, None, D],
           [S, -1, 0, 1, 0.0, None, None, None, None, D], [S, 10, 0, 1, 0.0, None, None, None, None, D], [T, 10, 0, 1, 0.0, A, A, A, A, None],
           [S, M.ATAN2, 0, 1, 0.0, None, None, None, None, D], [S, M.DIV, 0, 1, 0.0, None, None, None, None, D], [S, M.MULADD, 0, 1, 0.0, None, None, None, None, D],
           [S, M.LOG, 0, 1, 0.0, None, None, None, None, None], [S, M.LOG, 0, 1, 0.0, A, None, None, None, D], [S, M.LOG, 0, 1, 0.0, None, None, None, A, D],
           [S, M.LOG, 0, 0, 0.0, None, None, None, None, D], [S, M.LOG, 0, (1 << 32) + 1, 0.0, None, None, None, None, D],
           [S, M.LOG, 1, 1 << 32, 0.0, None, None, None, None, D], [S, M.LOG, 0xFFFFFFFF, 2, 0.0, None, None, None, None, D],
           [S, M.POW, 0, 1, 0.0, None, None, None, None, D], [S, M.POW, 0, 1, -2.2, None, None, None, None, D],
           [S, M.POW, 0, 1, float("inf"), None, None, None, None, D], [S, M.POW, 0, 1, float("nan"), None, None, None, None, D],
           [T, M.LOG, 0, 1, 0.0, None, None, None, A, None], [T, M.LOG, 0, 1, 0.0, A, None, None, None, None], [T, M.LOG, 0, 1, 0.0, A, None, None, A, D],
           [T, M.ATAN2, 0, 1, 0.0, A, None, None, A, None], [T, M.POW, 0, 1, 0.0, A, None, None, A, None], [T, M.DIV, 0, 1, 0.0, A, None, None, A, None],
           [T, M.MULADD, 0, 1, 0.0, A, A, None, A, None], [T, M.MULADD, 0, 1, 0.0, A, None, A, A, None],
           [T, M.LOG, 0, 0, 0.0, A, None, None, A, None], [T, M.LOG, 0, (1 << 24) + 1, 0.0, A, None, None, A, None], [T, M.LOG, 1, 1, 0.0, A, None, None, A, None]]
    for args in bad:
        st = L.rt_debug_math_tests(*args)
        text = L.rt_last_error_detail().decode()
        assert st == 1 and text.startswith("rt_debug_math_tests:"), (args[:5], st, text)
    if art._initialised_device is None:
        assert L.rt_debug_math_tests(S, M.LOG, 0, 1, 0.0, None, None, None, None, D) == 2      # RT_ERR_NO_DEVICE
        assert L.rt_debug_math_tests(T, M.MULADD, 0, 4, 0.0, A, A, A, A, None) == 2
