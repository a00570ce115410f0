"""What tests/test_device_math_host.py and tests/test_device_math.py share: the function ids of rt_debug_math_tests
(include/rt_abi.h), thin callers of its two forms, the digest restated in NumPy, mpmath as the arbiter of what the correctly
rounded float32 of a function's value is, the fixed samples, and the comparison of a swept range on the two sides.

The digest (include/rt_abi.h): per block of 2^20 consecutive words, the sum modulo 2^64 of mix64(word, result bits), mix64 being
the finaliser of splitmix64 over word * 2^32 + bits, every NaN result counted as 0x7FC00000.
"""
import time

import mpmath
import numpy as np

F = np.float32
LOG, SIN, ACOS, ATAN2, POW, POW5, SQRT, RCP, DIV, MULADD, POW5_PRODUCT = range(11)   # POW5_PRODUCT: the oracle's only
NAMES = ["log", "sin", "acos", "atan2", "pow", "pow5", "sqrt", "rcp", "div", "muladd", "pow5_product"]
SWEEP, LIST = 0, 1
BLOCK = 1 << 20
ONE, TWO, INF, TWO24 = 0x3F800000, 0x40000000, 0x7F800000, 0x4B800000   # float32 bit patterns
NEG = 0x80000000
PREC = 256                                                               # bits mpmath works with (the issue asks for 200 at least)


# ------------------------------------------------------------------ the two forms on the device
def dev_sweep(L, fn, first, count, operand=0.0):
    digests = np.zeros((count + BLOCK - 1) // BLOCK, np.uint64)
    st = L.rt_debug_math_tests(SWEEP, fn, first, count, operand, None, None, None, None, digests.ctypes.data)
    assert st == 0, L.rt_last_error_detail().decode()
    return digests


def dev_list(L, fn, a, b=None, c=None):
    a = np.ascontiguousarray(a, F)
    b, c = (None if x is None else np.ascontiguousarray(x, F) for x in (b, c))
    out = np.zeros(len(a), F)
    ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    st = L.rt_debug_math_tests(LIST, fn, 0, len(a), 0.0, ptr(a), ptr(b), ptr(c), out.ctypes.data, None)
    assert st == 0, L.rt_last_error_detail().decode()
    return out


# ------------------------------------------------------------------ the digest, restated
def canonical_bits(results):
    bits = np.ascontiguousarray(results, F).view(np.uint32).copy()
    bits[np.isnan(results)] = 0x7FC00000
    return bits


def mix64(words, bits):
    z = (np.asarray(words).astype(np.uint64) << np.uint64(32)) | np.asarray(bits).astype(np.uint64)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def digest(words, results):
    """The digest of one block: words (uint32) and the float32 results of the function on them."""
    return np.uint64(mix64(words, canonical_bits(results)).sum(dtype=np.uint64))


def words_as_floats(first, count):
    return np.arange(first, first + count, dtype=np.uint64).astype(np.uint32).view(F)


# ------------------------------------------------------------------ mpmath: the correctly rounded float32
def round_bits(v):
    """The bit pattern of the float32 nearest the mpf v, ties to even, subnormals and overflow included (+0 for a zero)."""
    if mpmath.isnan(v):
        return 0x7FC00000
    sign, man, exp, bc = v._mpf_
    if mpmath.isinf(v):
        return INF | (NEG if v < 0 else 0)
    if man == 0:
        return 0
    q = max(exp + bc - 1 - 23, -149)            # the exponent of the result's last place
    sh = exp - q
    if sh >= 0:
        n = man << sh
    else:
        n, rem, half = man >> -sh, man & ((1 << -sh) - 1), 1 << (-sh - 1)
        if rem > half or (rem == half and n & 1):
            n += 1
    if n == 1 << 24:
        n, q = n >> 1, q + 1
    if q + 23 > 127:
        bits = INF
    elif n < 1 << 23:
        bits = n                                 # subnormal, or zero
    else:
        bits = ((q + 23 + 127) << 23) | (n - (1 << 23))
    return bits | (NEG if sign else 0)


def exact(fn, a, b=0.0):
    """The function's value on float32 a (and b) as an mpf of PREC bits; the callers hold mpmath.workprec(PREC)."""
    A, B = mpmath.mpf(float(a)), mpmath.mpf(float(b))
    if fn == LOG:
        return mpmath.log(A) if A > 0 else (mpmath.mpf("-inf") if A == 0 else mpmath.nan)
    if fn == SIN:
        return mpmath.sin(A)
    if fn == ACOS:
        return mpmath.acos(A) if abs(A) <= 1 else mpmath.nan
    if fn == ATAN2:
        return mpmath.atan2(A, B)
    if fn == POW:                                # apply_gamma: 1 / gamma in float32, a negative colour clamps to 0
        if F(b) == F(1.0):
            return A
        inv = mpmath.mpf(float(F(1.0) / F(b)))
        x = A if A > 0 else mpmath.mpf(0)
        return x if (x == 0 or mpmath.isinf(x)) else mpmath.power(x, inv)
    if fn in (POW5, POW5_PRODUCT):
        return A ** 5
    if fn == SQRT:
        return mpmath.sqrt(A) if A >= 0 else mpmath.nan
    if fn == RCP:
        return 1 / A
    if fn == DIV:
        return A / B
    raise ValueError(fn)


def correct_bits(fn, a, b=None):
    """The correctly rounded float32 results, as bit patterns, for arrays of finite inputs; 0xFFFFFFFF where mpmath has no
    value (a division by zero).  mpmath has one zero: where atan2's answer hangs on a zero's sign, this is the answer for +0."""
    a = np.asarray(a, F)
    b = np.zeros(len(a), F) if b is None else np.asarray(b, F)
    out = np.zeros(len(a), np.uint32)
    with mpmath.workprec(PREC):
        for i in range(len(a)):
            try:
                bits = round_bits(exact(fn, a[i], b[i]))
            except ZeroDivisionError:
                bits = 0xFFFFFFFF
            if bits == 0 and fn in (SIN, POW5, POW5_PRODUCT, SQRT):
                bits = int(a[i:i + 1].view(np.uint32)[0]) & NEG   # an exact zero: sin(-0), (-0)^5 and sqrt(-0) keep the sign
            out[i] = bits
    return out


# ------------------------------------------------------------------ the fixed samples of the host test
N_SAMPLE = 4096


def edge_words():
    """0.5, 1 and every power of two of the normal range, and the floats one ulp either side of each."""
    w = np.array([(e << 23) + d for e in range(1, 255) for d in (-1, 0, 1)], np.int64)
    return w[(w > 0) & (w < INF)].astype(np.uint32)


def _fill(rng, fixed, lo, hi, signs):
    """`fixed` words, then random words of [lo, hi) (with random signs where `signs`), N_SAMPLE in all, none twice."""
    fixed = np.unique(fixed)[: N_SAMPLE // 2] if len(fixed) > N_SAMPLE // 2 else np.unique(fixed)
    extra = rng.integers(lo, hi, 4 * N_SAMPLE).astype(np.uint32)
    if signs:
        extra |= (rng.integers(0, 2, len(extra)).astype(np.uint32) << np.uint32(31))
    extra = extra[~np.isin(extra, fixed)]
    _, idx = np.unique(extra, return_index=True)
    extra = extra[np.sort(idx)]
    return np.concatenate([fixed, extra[: N_SAMPLE - len(fixed)]]).astype(np.uint32)


def sample(fn):
    """(a, b): 4096 fixed float32 inputs of fn's domain -- the edge words, then random bit patterns (seeded)."""
    rng = np.random.default_rng(20261020 + fn)
    e = edge_words()
    if fn == LOG:
        a, b = _fill(rng, e, 1, INF, False), None
    elif fn == SIN:
        a, b = _fill(rng, np.concatenate([e, e | np.uint32(NEG)]), 1, INF, True), None
    elif fn == ACOS:
        e = e[e <= ONE]
        a, b = _fill(rng, np.concatenate([e, e | np.uint32(NEG)]), 1, ONE + 1, True), None
    elif fn == ATAN2:
        a = _fill(rng, np.concatenate([e, e | np.uint32(NEG)]), 1 << 23, INF, True)
        b = rng.permutation(_fill(rng, np.concatenate([e, e | np.uint32(NEG)]), 1 << 23, INF, True))
        v = rng.normal(size=(N_SAMPLE // 4, 3))                                    # a quarter: (-p.z, p.x) of unit vectors
        v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
        a[-len(v):], b[-len(v):] = (-v[:, 2]).view(np.uint32), v[:, 0].view(np.uint32)
        b = b.view(F)
    elif fn == POW:
        a = _fill(rng, e, 1, INF, False)
        b = np.array([2.2, 1.8, 2.0, 2.4], F)[np.arange(N_SAMPLE) % 4]
    elif fn in (POW5, POW5_PRODUCT):
        a, b = _fill(rng, e[e <= TWO], 1, TWO + 1, False), None
    else:
        raise ValueError(fn)
    assert len(a) == N_SAMPLE
    return a.view(F), b


# ------------------------------------------------------------------ a swept range on both sides
def describe(fn, a, b, dev, orc_r):
    """One record per input on which the two sides disagree: the input bits, both results, mpmath's correctly rounded value and
    which side that faults."""
    right = correct_bits(fn, a, b) if fn != MULADD else np.zeros(len(a), np.uint32)    # a * b + c of the tests: +0 as written
    recs = []
    for i in range(len(a)):
        d, o = (int(canonical_bits(x[i:i + 1])[0]) for x in (dev, orc_r))
        who = "device" if o == right[i] != d else "oracle" if d == right[i] != o else "both"
        rec = {"fn": NAMES[fn], "a": f"0x{int(a[i:i + 1].view(np.uint32)[0]):08X}", "device": f"0x{d:08X}", "oracle": f"0x{o:08X}",
               "correct": f"0x{int(right[i]):08X}", "wrong": who}
        if b is not None:
            rec["b"] = f"0x{int(b[i:i + 1].view(np.uint32)[0]):08X}"
        recs.append(rec)
    return recs


def compare_lists(L, orc, fn, a, b=None, c=None):
    """The list form on both sides, element by element: the records of the inputs on which the float results' bits differ."""
    dev, ref = dev_list(L, fn, a, b, c), orc.math_list(fn, a, b, c)
    bad = np.flatnonzero(canonical_bits(dev) != canonical_bits(ref))
    return describe(fn, a[bad], None if b is None else b[bad], dev[bad], ref[bad]) if len(bad) else []


def compare_sweep(L, orc, fn, first, count, operand=0.0, max_blocks=None):
    """Both sweeps over words first .. first + count - 1.  Returns (blocks that differ, records of every disagreeing input of the
    first max_blocks of them -- all of them for None --, seconds on the device, seconds on the oracle)."""
    t0 = time.perf_counter()
    dev = dev_sweep(L, fn, first, count, operand)
    t1 = time.perf_counter()
    ref = orc.math_sweep(fn, first, count, operand)
    t2 = time.perf_counter()
    differ = np.flatnonzero(dev != ref)
    recs = []
    for k in differ[:max_blocks]:
        w0 = first + int(k) * BLOCK
        n = min(BLOCK, first + count - w0)
        a = words_as_floats(w0, n)
        found = compare_lists(L, orc, fn, a, np.full(n, operand, F) if fn == POW else None)
        assert found, (NAMES[fn], hex(w0), "the digests differ and the lists do not")
        recs += found
    return len(differ), recs, t1 - t0, t2 - t1
