"""The ranking's host reference (tests/rank_expect.py) and the four diagnostic entries, without a device: the reference against
values worked out by hand, its own outputs against the order-free assertions the device's outputs must meet, the branch outcomes
the cases of tests/test_rank.py reach, and the argument checks that run before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import rank_expect as rx

RT_ERR_INVALID, RT_ERR_NO_DEVICE = 1, 2
FAKE = 0x1000   # never dereferenced: every check below fails before a pointer is looked at
NONE = 0xFFFFFFFF
CASES = rx.rank_cases()


def test_debug_entries_are_exported(art):
    for sym in ("rt_debug_rank", "rt_debug_prior", "rt_debug_cal_cost", "rt_debug_rank_info"):
        assert sym in art.RT_ABI_SYMBOLS
        assert hasattr(art.rt_lib(), sym)


# ------------------------------------------------------------------------------------------------- the reference, worked by hand
def _hand_params(n_pixels, nx, **over):
    """One tile; factors 1.5 / 2.0 / 3.0 (list / sparse / tier 1); a grid of 10 workgroups of 8 waves, half of it for sparse and
    semi workgroups; tier 1: up to 16 pixels, one per wave, four workgroups; the whole work may go to the tiers."""
    p = dict(n_pixels=n_pixels, n_tiles=1, heavy_cap=8, max_grid=10, waves_per_wg=8, normal_need=1, sparse_stride=8, semi_stride=1,
             sparse_percent=50, sparse_work_percent=100, tier_possible=1, tier1_pixels=16, tier1_depth=1, tier_wgs_cap=4,
             tier_waves_per_main_wg=0, nx=nx, smooth_percent=0, heavy_factor=1.5, sparse_factor=2.0, tier1_factor=3.0)
    p.update(over)
    return p


# words: heavy_items, heavy_threshold, tier1_items, tier2_items, tier1_wgs, main_skip_wgs, sparse_wgs, sparse_stride, semi_wgs,
#        semi_stride, threshold1, threshold2, collected.
# Four pixels cost 200 rays, mean 50: the list starts at int(75.999) = 75, tier 2 at int(100.999) = 100, tier 1 at int(150.999) = 150.
HAND = {
    # one pixel at 170 is listed and reaches tier 1; its bucket's midpoint 170 - 0.5 / 2048 is within the budget of 200 rays; one
    # tier workgroup, nothing left for tiers 2 and 3, so no sparse or semi workgroup
    "four pixels, one dear": (_hand_params(4, 2), [10, 10, 10, 170], 200, [1, 75, 1, 0, 1, 0, 0, 8, 0, 1, 150, 100, 1]),
    # ... with half the work as budget (100 rays) its 169.9998 rays are not admitted: it stays tier 3, which takes one semi workgroup
    "four pixels, one dear, not admitted": (_hand_params(4, 2, sparse_work_percent=50), [10, 10, 10, 170], 200,
                                            [1, 75, 0, 0, 0, 0, 0, 8, 1, 1, 150, 100, 1]),
    # nobody reaches 75
    "all costs equal": (_hand_params(4, 2), [50, 50, 50, 50], 200, [0, NONE, 0, 0, 0, 0, 0, 1, 0, 1, 150, 100, 0]),
    # every threshold is int(0.999) = 0, every pixel is collected, and all of them are more than half
    "total zero": (_hand_params(4, 2), [0, 0, 0, 0], 0, [0, NONE, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 4]),
    # eight pixels, 400 rays, two at 170: both tier 1 (2 x 169.9998 <= 400), one tier workgroup -- if the list holds two
    "count == heavy_cap": (_hand_params(8, 4, heavy_cap=2), [10, 10, 10, 170, 10, 170, 10, 10], 400, [2, 75, 2, 0, 1, 0, 0, 8, 0, 1, 150, 100, 2]),
    "count == heavy_cap + 1": (_hand_params(8, 4, heavy_cap=1), [10, 10, 10, 170, 10, 170, 10, 10], 400, [0, NONE, 0, 0, 0, 0, 0, 1, 0, 1, 150, 100, 2]),
    # two of four pixels at 90: half the pixels is not a list
    "2 * count == n_pixels": (_hand_params(4, 2), [10, 90, 10, 90], 200, [0, NONE, 0, 0, 0, 0, 0, 1, 0, 1, 150, 100, 2]),
    # no sparse waves, no heavy threshold, nothing collected; the tier thresholds are computed all the same
    "sparse_stride == 0": (_hand_params(4, 2, sparse_stride=0), [10, 10, 10, 170], 200, [0, NONE, 0, 0, 0, 0, 0, 1, 0, 1, 150, 100, 0]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_reference_matches_hand_worked_cases(name):
    p, cost, total, words = HAND[name]
    info, _ = rx.rank_info(p, np.array(cost, np.uint32), total)
    assert rx.info_words(info) == words


def test_reference_pieces_by_hand():
    assert rx.thresholds(200, 4, (1.5, 2.0, 3.0), 8) == (75, 150, 100)
    assert rx.thresholds(200, 4, (1.5, 2.0, 3.0), 0) == (NONE, 150, 100)
    assert rx.thresholds(1001, 10, (2.0, 4.0, 4.5), 8) == (201, 451, 401)      # 200.2 + 0.999, 450.9 + 0.999, 400.4 + 0.999
    assert rx.thresholds(1000, 10, (2.0, 4.0, 4.5), 8) == (200, 450, 400)      # an exact product stays: + 0.999, not + 1
    # 3 x 2 pixels; the middle of the top row is dear and carries a stale flag: its neighbours get 90 % of it, the corner below only sees them
    cost = np.array([5, 0x80000000 | 100, 7, 1, 2, 200], np.uint32)
    assert rx.estimates(cost, 3, 0).tolist() == [5, 100, 7, 1, 2, 200]
    assert rx.estimates(cost, 3, 90).tolist() == [90, 100, 180, 4, 180, 200]
    assert rx.estimates(cost, 3, 100).tolist() == [100, 100, 200, 5, 200, 200]
    pixels, new_cost, collected = rx.listing(cost, rx.estimates(cost, 3, 90), 100)
    assert pixels.tolist() == [1, 2, 4, 5] and collected == 4
    assert new_cost.tolist() == [5, 0x80000000 | 100, 0x80000000 | 7, 1, 0x80000000 | 2, 0x80000000 | 200]
    assert rx.listing(cost, rx.estimates(cost, 3, 0), 101)[1].tolist() == [5, 100, 7, 1, 2, 0x80000000 | 200]   # a stale flag is cleared
    # buckets: the dearest key in bucket 0, the cheapest in the last one a span allows
    assert [rx.bucket(k, 0, 2047) for k in (2047, 2046, 1, 0)] == [0, 1, 2046, 2047]
    assert [rx.bucket(k, 10, 12) for k in (12, 11, 10)] == [0, 682, 1365]
    assert rx.bucket(7, 7, 7) == 0
    assert rx.bucket(0, 0, 0x7FFFFFFF) == 2047 and rx.bucket(0x7FFFFFFF - (1 << 20), 0, 0x7FFFFFFF) == 1
    h = rx.cumulative_histogram([12, 12, 11, 10, 10, 10])
    assert h[0] == 2 and h[681] == 2 and h[682] == 3 and h[1364] == 3 and h[1365] == 6 and h[2047] == 6 and len(h) == 2048


def test_prior_reference_by_hand():
    """A 4 x 3 calibration grid under a 10 x 7 frame of which the call renders bands 1 and 3 of two rows: global rows 2, 3 and 6.
    Columns 0..9 fall on calibration columns 0 0 0 1 1 2 2 2 3 3, rows 2, 3, 6 on calibration rows 0, 1, 2."""
    cal = np.array([[40, 2, 3, 4],
                    [8, 7, 6, 5],
                    [9, 20, 11, 30]], np.uint32)
    cost, tile_cost, total = rx.prior(cal, 10, 7, 2, 1, 2)
    assert rx.local_rows(7, 2, 1, 2) == 3
    assert [rx.local_to_global_row(r, 2, 1, 2) for r in range(3)] == [2, 3, 6]
    assert cost.tolist() == [[40, 40, 40, 40, 40, 7, 7, 7, 6, 6],        # calibration rows 0..1
                             [40, 40, 40, 40, 40, 30, 30, 30, 30, 30],   # rows 0..2
                             [20, 20, 20, 20, 20, 30, 30, 30, 30, 30]]   # rows 1..2
    assert tile_cost.tolist() == [701, 132] and total == 833


# --------------------------------------------------------------------------------------- the reference on the device tests' inputs
@pytest.mark.parametrize("name,inputs", CASES, ids=[c[0] for c in CASES])
def test_reference_outputs_meet_the_order_free_assertions(name, inputs):
    out = rx.reference_outputs(inputs)
    rx.check_rank_outputs(inputs, out)


def test_check_rank_outputs_refuses_wrong_outputs():
    """The order-free assertions are not vacuous: an ascending order, a missing or doubled pixel, a wrong flag, a tier beyond its
    workgroups each fail them."""
    name, inputs = CASES[0]
    good = rx.reference_outputs(inputs)
    n = good["info"][0]
    assert n > 4

    def broken(**change):
        out = {k: (v.copy() if isinstance(v, np.ndarray) else list(v) if isinstance(v, list) else v) for k, v in good.items()}
        for k, f in change.items():
            out[k] = f(out[k])
        with pytest.raises(AssertionError):
            rx.check_rank_outputs(inputs, out)

    def reverse_list(h):
        h[:n] = h[:n][::-1].copy()
        return h

    def double(h):
        h[1] = h[0]
        return h

    def flag(c):
        c[int(np.flatnonzero((c & 0x80000000) == 0)[0])] |= 0x80000000
        return c

    def low_bits(c):
        c[0] += 1
        return c

    def word(k, v):
        def f(info):
            info[k] = v
            return info
        return f

    broken(tile_order=lambda t: t[::-1].copy())
    broken(tile_order=lambda t: np.where(t == 3, 4, t).astype(np.uint32))
    broken(heavy_pixels=reverse_list)
    broken(heavy_pixels=double)
    broken(cost_out=flag)
    broken(cost_out=low_bits)
    broken(info=word(0, n - 1))
    broken(info=word(1, good["info"][1] + 1))
    broken(info=word(3, n))                       # tier 2 beyond the list and beyond its workgroups
    broken(info=word(4, 0))                       # tier-1 items without a tier workgroup
    broken(info=word(5, 10 ** 6))
    broken(info=word(6, 10 ** 6))


def test_cases_reach_every_branch_outcome():
    """Every item of the issue's parameter list occurs in the cases, and the reference takes every branch outcome at least once."""
    seen = set()
    for name, inputs in CASES:
        seen |= rx.rank_info(inputs["params"], inputs["cost"], inputs["total"])[1]
    assert seen == set(rx.OUTCOMES), set(rx.OUTCOMES) - seen
    ps = [c[1]["params"] for c in CASES]
    for key, values in {"sparse_stride": (0, 2, 8, 64), "semi_stride": (0, 1, 4), "tier_possible": (0, 1), "tier1_pixels": (0, 256, 1536, 8192),
                        "tier1_depth": (1, 3, 4), "tier_waves_per_main_wg": (0, 3, 4), "sparse_work_percent": (1, 5, 40, 100),
                        "smooth_percent": (0, 90, 100)}.items():
        assert set(values) <= {p[key] for p in ps}, key
    assert {(p["nx"], p["n_pixels"] // p["nx"]) for p in ps} == set(rx.SIZES)
    assert any(c[1]["total"] == 2 * int((c[1]["cost"].astype(np.int64) & rx.MASK).sum()) > 0 for c in CASES)
    collected = [rx.rank_info(c[1]["params"], c[1]["cost"], c[1]["total"])[0]["collected"] for c in CASES]
    assert any(n > p["heavy_cap"] for n, p in zip(collected, ps)) and any(n == p["heavy_cap"] for n, p in zip(collected, ps))
    assert any(n > 1024 for n in collected)                            # a list longer than one pass of the workgroup's loops
    assert any(2 * n >= p["n_pixels"] > n > 0 for n, p in zip(collected, ps))
    assert any(0 < p["n_pixels"] - 2 * n < p["n_pixels"] // 100 for n, p in zip(collected, ps))   # just under half the pixels: still a list


def test_edges_field_sits_on_the_thresholds():
    """The "edges" field has estimates exactly on, one below and one above each threshold of its parameter set."""
    hits = 0
    for name, inputs in CASES:
        if "-edges-" not in name:
            continue
        p = inputs["params"]
        ts = rx.thresholds(inputs["total"], p["n_pixels"], (p["heavy_factor"], p["sparse_factor"], p["tier1_factor"]), p["sparse_stride"])
        est = set(rx.estimates(inputs["cost"], p["nx"], p["smooth_percent"]).tolist())
        for t in ts:
            assert {t - 1, t, t + 1} <= est, (name, t)
        hits += 1
    assert hits >= 3


# ------------------------------------------------------------------------------------------------------------ argument checks
def _rank_args(**over):
    p = rx.base_params(8, 8, "lean")
    p.update({k: v for k, v in over.items() if k in p})
    n, cap = 64, 262144
    bufs = {"cost": np.zeros(n, np.uint32), "tile_cost": np.zeros(1, np.uint32), "params": rx.pack_params(p), "tile_order": np.zeros(1, np.uint32),
            "cost_out": np.zeros(n, np.uint32), "heavy_pixels": np.zeros(cap, np.uint32), "info": np.zeros(13, np.uint32)}
    ptr = {k: (None if over.get(k, 1) is None else v.ctypes.data) for k, v in bufs.items()}
    return bufs, [ptr["cost"], ptr["tile_cost"], over.get("rays", 100), ptr["params"], ptr["tile_order"], ptr["cost_out"], ptr["heavy_pixels"], ptr["info"]]


def test_debug_rank_argument_checks(art):
    L = art.rt_lib()
    inf, nan = float("inf"), float("nan")
    bad = [dict(cost=None), dict(tile_cost=None), dict(params=None), dict(tile_order=None), dict(cost_out=None), dict(heavy_pixels=None), dict(info=None),
           dict(n_pixels=0), dict(n_pixels=1 << 31), dict(n_tiles=0), dict(n_tiles=65), dict(heavy_cap=0), dict(heavy_cap=(1 << 24) + 1),
           dict(max_grid=(1 << 20) + 1), dict(normal_need=(1 << 20) + 1), dict(waves_per_wg=0), dict(waves_per_wg=17),
           dict(sparse_stride=-1), dict(sparse_stride=65), dict(semi_stride=-1), dict(semi_stride=65), dict(sparse_percent=101), dict(sparse_percent=-1),
           dict(sparse_work_percent=101), dict(smooth_percent=101), dict(smooth_percent=-1), dict(tier1_pixels=-1), dict(tier1_depth=-1),
           dict(tier1_depth=65537), dict(tier_wgs_cap=-1), dict(tier_waves_per_main_wg=-1), dict(nx=0), dict(nx=65),
           dict(heavy_factor=-1.0), dict(sparse_factor=nan), dict(tier1_factor=inf), dict(tier1_factor=1001.0), dict(rays=1 << 40)]
    for over in bad:
        bufs, args = _rank_args(**over)
        st = L.rt_debug_rank(*args)
        text = L.rt_last_error_detail().decode()
        assert st == RT_ERR_INVALID and text.startswith("rt_debug_rank:"), (over, st, text)
    if art._initialised_device is None:      # what passes every check gets as far as the device, and no further
        bufs, args = _rank_args()
        assert L.rt_debug_rank(*args) == RT_ERR_NO_DEVICE


def _prior_args(**over):
    a = dict(cal=np.zeros(12, np.uint32), cal_nx=4, cal_ny=3, nx=10, ny=7, tile_rows=2, tile_first=1, tile_stride=2, cost=np.zeros(30, np.uint32),
             tile_cost=np.zeros(2, np.uint32), total=C.c_uint64(0))
    a.update(over)
    ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    return a, [ptr(a["cal"]), a["cal_nx"], a["cal_ny"], a["nx"], a["ny"], a["tile_rows"], a["tile_first"], a["tile_stride"], ptr(a["cost"]),
               ptr(a["tile_cost"]), None if a["total"] is None else C.byref(a["total"])]


def test_debug_prior_argument_checks(art):
    L = art.rt_lib()
    bad = [dict(cal=None), dict(cost=None), dict(tile_cost=None), dict(total=None), dict(cal_nx=0), dict(cal_ny=-1), dict(cal_nx=1 << 16, cal_ny=1 << 15),
           dict(nx=0), dict(ny=0), dict(nx=1 << 16, ny=1 << 15), dict(tile_rows=0), dict(tile_stride=0), dict(tile_first=-1), dict(tile_first=4)]
    for over in bad:
        keep, args = _prior_args(**over)
        st = L.rt_debug_prior(*args)
        text = L.rt_last_error_detail().decode()
        assert st == RT_ERR_INVALID and text.startswith("rt_debug_prior:"), (over, st, text)
    if art._initialised_device is None:
        keep, args = _prior_args()
        assert L.rt_debug_prior(*args) == RT_ERR_NO_DEVICE


def test_debug_scene_entries_argument_checks(art):
    """Null scene, null outputs and a cap below the smallest calibration grid (8 x 8) are refused before the scene is looked at."""
    L = art.rt_lib()
    out = np.zeros(64, np.uint32)
    nx, ny = C.c_int32(-5), C.c_int32(-5)
    for scene, o, cap, px, py in [(None, out.ctypes.data, 64, C.byref(nx), C.byref(ny)), (FAKE, None, 64, C.byref(nx), C.byref(ny)),
                                  (FAKE, out.ctypes.data, 64, None, C.byref(ny)), (FAKE, out.ctypes.data, 64, C.byref(nx), None),
                                  (FAKE, out.ctypes.data, 0, C.byref(nx), C.byref(ny)), (FAKE, out.ctypes.data, 63, C.byref(nx), C.byref(ny)),
                                  (FAKE, out.ctypes.data, -1, C.byref(nx), C.byref(ny))]:
        st = L.rt_debug_cal_cost(scene, o, cap, px, py)
        text = L.rt_last_error_detail().decode()
        assert st == RT_ERR_INVALID and text.startswith("rt_debug_cal_cost:"), (scene, cap, st, text)
    assert (nx.value, ny.value) == (-5, -5) and not out.any()
    for scene, o in [(None, out.ctypes.data), (FAKE, None)]:
        st = L.rt_debug_rank_info(scene, o)
        text = L.rt_last_error_detail().decode()
        assert st == RT_ERR_INVALID and text.startswith("rt_debug_rank_info:"), (scene, st, text)
    assert "null scene" in text or "null argument" in text
