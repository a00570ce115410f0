"""The order of the tail hand-off queue (csrc/rt_handoff_order.h): between the main kernel and the tail launch the
queue is copied into a second buffer, entries with the most remaining work first.  Scheduling only: frames and ray counts are
the oracle's with the option on and off, whoever finishes the pixels; the ordering launch itself (rt_debug_order_handoff)
returns a permutation of its input in non-increasing bucket order, or the input where it copies through."""
import numpy as np
import pytest

import accelerated_ray_tracer_amd as art_host   # the NumPy restatement needs no GPU

NS = 32
SCENES = ("bouncing", "cornell", "final")            # the lean family; scan mode; general
BAND = dict(tile_rows=8, tile_first=1, tile_stride=2)
# every pixel handed off after its first sample, in frames of several parts so that parked costs count from sample 0 too
ALL_HANDED = {"handoff_pixels": 1 << 24, "handoff_poll_us": 1}
_cache = {}


def _case(art, orc, name, nx=64, ny=64):
    """The scene, the oracle's frame and its ray counts row by row; made once per scene and size."""
    key = (name, nx, ny)
    if key not in _cache:
        img, iw, ih = art.default_texture(name)
        hs = art.HostScene(name, nx, ny, img, iw, ih)
        o = orc.OracleScene(name, nx, ny, img, iw, ih)
        ref, cnt = o.render(NS)
        band_rows = art.local_rows_to_global(hs.frame(ns=NS, **BAND))
        band_rays = sum(o.render(NS, row0=int(j), row1=int(j) + 1)[1]["rays"] for j in band_rows)
        _cache[key] = dict(hs=hs, ref=ref, rays=cnt["rays"], band_rows=band_rows, band_rays=band_rays)
    return _cache[key]


def _same(got, want, what):
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} values differ, first at {bad[:3].tolist()}"


def _check_served(entries, costs, served, info, sample_begin, what):
    """What the tail launch was given: the pushed entries, each once; in bucket order where the count is inside the limits."""
    assert np.array_equal(np.sort(served), np.sort(entries)), what
    if info["ordered"] and info["min"] <= len(entries) <= info["max"]:
        cost_of = dict(zip(entries.tolist(), costs.tolist()))
        b = art_host.handoff_order_bucket(art_host.handoff_order_key(served, [cost_of[e] for e in served.tolist()], sample_begin, NS))
        assert (np.diff(b) <= 0).all(), what
    else:
        assert np.array_equal(served, entries), what


@pytest.mark.gpu
@pytest.mark.parametrize("handed", ["auto", "all"])
@pytest.mark.parametrize("name", SCENES)
def test_frames_match_the_oracle_ordered_or_not(gpu, orc, name, handed):
    """64x64 @ 32, the smallest frame the ranked schedule accepts, cold (several parts) and warm (ranked on the cost map): the whole
    frame and one row band, handoff_order 0 and 1, bit for bit the oracle's and each other's, with the oracle's ray counts."""
    c = _case(gpu, orc, name)
    frames = {}
    for order in (0, 1):
        gpu.reset_options()
        for k, v in (ALL_HANDED if handed == "all" else {}).items():
            gpu.set_option(k, v)
        gpu.set_option("handoff_order", order)
        ds = gpu.DeviceScene(c["hs"])
        try:
            for temp in ("cold", "warm"):
                what = f"{name} {handed} handoff_order={order} {temp}"
                fb, st = ds.render(c["hs"].frame(ns=NS))
                assert st.rays == c["rays"], (what, st.rays, c["rays"])
                _same(fb, c["ref"], what)
                entries, costs, served, info = ds.handoff_queue()
                assert info["ordered"] == bool(order), what
                if handed == "all":
                    assert len(entries) > 0, what
                # (a warm frame is one fresh part from sample 0, or its last part resumes parked pixels: costs count from 0 either way)
                _check_served(entries, costs, served, info, 0, what)
                frames[(order, temp)] = fb
            band, st = ds.render(c["hs"].frame(ns=NS, **BAND))
            assert st.rays == c["band_rays"], (name, handed, order, "band")
            _same(band, c["ref"][c["band_rows"]], f"{name} {handed} handoff_order={order} band")
            frames[(order, "band")] = band
        finally:
            ds.close()
    for temp in ("cold", "warm", "band"):
        _same(frames[(0, temp)], frames[(1, temp)], f"{name} {handed} {temp}: handoff_order 0 against 1")


@pytest.mark.gpu
def test_a_frame_whose_queue_is_ordered(gpu, orc):
    """A 64x64 frame's queue stays below two entries per tail wave and is copied through.  256x64 with every pixel handed off
    fills the queue to where the ordering runs, in whole frames and in a row band of 64 tiles: the frames are the oracle's,
    and the queue the tail launch was given is the pushed queue in bucket order."""
    c = _case(gpu, orc, "bouncing", 256, 64)
    for k, v in ALL_HANDED.items():
        gpu.set_option(k, v)
    ds = gpu.DeviceScene(c["hs"])
    try:
        ordered_runs = 0
        for temp in ("cold", "warm"):
            fb, st = ds.render(c["hs"].frame(ns=NS))
            assert st.rays == c["rays"], temp
            _same(fb, c["ref"], temp)
            entries, costs, served, info = ds.handoff_queue()
            assert info["ordered"] and len(entries) > 0
            _check_served(entries, costs, served, info, 0, temp)
            ordered_runs += info["min"] <= len(entries) <= info["max"]
        assert ordered_runs > 0, (len(entries), info)
        band, st = ds.render(c["hs"].frame(ns=NS, **BAND))
        assert st.rays == c["band_rays"]
        _same(band, c["ref"][c["band_rows"]], "band")
        _check_served(*ds.handoff_queue(), 0, "band")
    finally:
        ds.close()


# ---- the ordering launch alone
TAIL_WAVES = 16                                      # ordered from 32 to 512 entries
LIMIT = art_host.HANDOFF_ORDER_MAX_PER_WAVE * TAIL_WAVES
COUNTS = (0, 1, 63, 64, 65, 1000, LIMIT - 1, LIMIT, LIMIT + 1)
SAMPLE_END = 1 << 20


def _entries(kind, n):
    """n entries with distinct pixels in shuffled order, and costs[pixel]."""
    rng = np.random.default_rng(1000 * n + len(kind))
    pix = rng.permutation(n).astype(np.uint64)
    costs = np.zeros(n, np.uint32)
    if kind == "equal":                               # all keys equal
        nxt = np.full(n, 100, np.uint64)
        costs[:] = 299
    elif kind == "mixed":                             # keys over many octaves, listed flags (bit 31) set on some, a few entries at their end
        nxt = rng.integers(0, SAMPLE_END, n).astype(np.uint64)
        costs[:] = (2.0 ** rng.uniform(0, 31, n)).astype(np.uint64).clip(0, 2 ** 31 - 1).astype(np.uint32)
        costs[rng.random(n) < 0.3] |= np.uint32(1 << 31)
        nxt[rng.random(n) < 0.1] = SAMPLE_END         # next == sample_end: nothing to go, key 0
    elif kind == "extreme":                           # one huge key, 2^51: a 2^31 - 1 cost with 2^20 samples to go (a 32-bit product loses it); the rest small
        nxt = rng.integers(1, 64, n).astype(np.uint64)
        costs[:] = rng.integers(0, 1000, n)
        if n:
            nxt[n // 2] = 0
            costs[pix[n // 2]] = 2 ** 31 - 1
    return (nxt << np.uint64(32)) | pix, costs, pix


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["equal", "mixed", "extreme"])
@pytest.mark.parametrize("n", COUNTS)
def test_ordering_is_a_permutation_in_bucket_order(gpu, n, kind):
    entries, costs, pix = _entries(kind, n)
    out, overrun = gpu.debug_order_handoff(entries, costs, 0, SAMPLE_END, TAIL_WAVES)
    assert overrun == 0                               # the push counter stands beyond the queue's end: the count is clipped
    assert np.array_equal(np.sort(out), np.sort(entries))
    if n < art_host.HANDOFF_ORDER_MIN_PER_WAVE * TAIL_WAVES or n > LIMIT:
        assert np.array_equal(out, entries)           # copied through
        return
    keys = art_host.handoff_order_key(out, costs[(out & np.uint64(0xFFFFFFFF)).astype(np.int64)], 0, SAMPLE_END)
    b = art_host.handoff_order_bucket(keys)
    assert (np.diff(b) <= 0).all(), np.flatnonzero(np.diff(b) > 0)[:5]
    if kind == "extreme":
        assert int(keys[0]) == (1 << 20) * (1 << 31) and b[0] == 1 + 4 * 51 and int(out[0]) == int(entries[n // 2])
    if kind == "equal":
        assert len(set(b.tolist())) == 1
    if kind == "mixed":
        assert len(set(b.tolist())) > min(n, 20) // 2  # the order was not trivially true


@pytest.mark.gpu
def test_ordering_counts_samples_from_sample_begin(gpu):
    """A middle sample range: "samples done" counts from sample_begin, and an entry past the end has nothing to go."""
    n = 200
    rng = np.random.default_rng(5)
    pix = rng.permutation(n).astype(np.uint64)
    nxt = rng.integers(40, 104, n).astype(np.uint64)       # [40, 100): some at the end, some beyond it
    costs = rng.integers(0, 5000, n).astype(np.uint32)
    entries = (nxt << np.uint64(32)) | pix
    out, overrun = gpu.debug_order_handoff(entries, costs, 40, 100, TAIL_WAVES)
    assert overrun == 0 and np.array_equal(np.sort(out), np.sort(entries))
    b = art_host.handoff_order_bucket(art_host.handoff_order_key(out, costs[(out & np.uint64(0xFFFFFFFF)).astype(np.int64)], 40, 100))
    assert (np.diff(b) <= 0).all() and b[-1] == 0 and b[0] > 0


@pytest.mark.gpu
def test_ordering_seam_refuses_bad_arguments(gpu):
    e, c = np.array([5], np.uint64), np.array([1], np.uint32)
    with pytest.raises(gpu.RtError):
        gpu.debug_order_handoff(e, c, 0, 10, TAIL_WAVES)       # pixel 5 of 1
    with pytest.raises(gpu.RtError):
        gpu.debug_order_handoff(np.array([0], np.uint64), c, 10, 5, TAIL_WAVES)
    with pytest.raises(gpu.RtError):
        gpu.debug_order_handoff(np.array([0], np.uint64), c, 0, 10, 0)


# ---- host: the NumPy restatement against hand-computed keys
def test_bucket_function_at_octave_boundaries():
    B = art_host.handoff_order_bucket
    # key 0 alone in bucket 0; below 4 the two sub-bits are shifted up: 1 -> (e 0, m 0), 2 -> (1, 0), 3 -> (1, 2)
    assert B([0, 1, 2, 3]).tolist() == [0, 1, 5, 7]
    # four buckets an octave: [4, 8) -> 9 .. 12, [8, 16) in steps of two -> 13 .. 16
    assert B([4, 5, 6, 7]).tolist() == [9, 10, 11, 12]
    assert B([8, 9, 10, 11, 12, 13, 14, 15]).tolist() == [13, 13, 14, 14, 15, 15, 16, 16]
    for e in (3, 10, 31, 32, 33, 61, 62):
        lo = 1 << e
        assert B([lo - 1, lo, lo + (lo >> 2) - 1, lo + (lo >> 2), 2 * lo - 1]).tolist() == [4 * e, 4 * e + 1, 4 * e + 1, 4 * e + 2, 4 * e + 4], e
    assert B([(1 << 64) - 1]).tolist() == [art_host.HANDOFF_BUCKETS - 1]
    ks = [int(k) for k in np.unique((2.0 ** np.random.default_rng(3).uniform(0, 62, 500)).astype(np.uint64))]
    assert (np.diff(B(ks)) >= 0).all()                 # monotone in the key


def test_key_is_the_issue_formula():
    K = art_host.handoff_order_key
    e = lambda nxt, pix: (nxt << 32) | pix             # noqa: E731
    # (500 - 100) * (299 + 1) // (100 + 1) = 1188; the listed flag (bit 31) is not part of the cost
    assert K([e(100, 7)], [299], 0, 500).tolist() == [1188]
    assert K([e(100, 7)], [299 | 1 << 31], 0, 500).tolist() == [1188]
    # samples done count from sample_begin: (500 - 100) * 300 // (100 - 64 + 1) = 3243
    assert K([e(100, 7)], [299], 64, 500).tolist() == [3243]
    # nothing to go at or past the end; nothing done at the start: 500 * (0 + 1) // 1
    assert K([e(500, 1), e(501, 2), e(0, 3)], [10, 10, 0], 0, 500).tolist() == [0, 0, 500]
    # the product needs 64 bits: 2^20 samples to go at a 2^31 - 1 cost
    assert K([e(0, 0)], [2 ** 31 - 1], 0, 1 << 20).tolist() == [1 << 51]
    # the largest key there is: 2^31 - 1 samples to go at a 2^31 - 1 cost, leading bit 61 and both sub-bits set
    top = K([e(0, 0)], [2 ** 31 - 1], 0, 2 ** 31 - 1)
    assert top.tolist() == [(2 ** 31 - 1) << 31] and art_host.handoff_order_bucket(top).tolist() == [1 + 4 * 61 + 3]
