"""The device-side ranking and the cost prior (csrc/rt_rank.hip) against the host reference of tests/rank_expect.py, through the
diagnostic entries rt_debug_rank / rt_debug_prior / rt_debug_cal_cost / rt_debug_rank_info (include/rt_abi.h).

The ranking is scheduling only -- no pixel changes when it is wrong, only the frame time -- so nothing else in the suite sees
its outputs.  Here they are compared word for word: the 13 words of rt_rank_info and the flagged costs exactly, the two sorted
orders up to what the sorts leave free (positions inside one of their 2048 buckets; rank_expect.check_rank_outputs)."""
import ctypes as C

import numpy as np
import pytest

import rank_expect as rx

pytestmark = pytest.mark.gpu

CASES = rx.rank_cases()


def device_rank(gpu, inputs) -> dict:
    p = inputs["params"]
    words = rx.pack_params(p)
    cost = np.ascontiguousarray(inputs["cost"], np.uint32)
    tile_cost = np.ascontiguousarray(inputs["tile_cost"], np.uint32)
    assert len(cost) == p["n_pixels"] and len(tile_cost) == p["n_tiles"]
    out = {"tile_order": np.zeros(p["n_tiles"], np.uint32), "cost_out": np.zeros(p["n_pixels"], np.uint32),
           "heavy_pixels": np.zeros(p["heavy_cap"], np.uint32), "info": np.zeros(13, np.uint32)}
    L = gpu.rt_lib()
    st = L.rt_debug_rank(cost.ctypes.data, tile_cost.ctypes.data, inputs["total"], words.ctypes.data, out["tile_order"].ctypes.data,
                         out["cost_out"].ctypes.data, out["heavy_pixels"].ctypes.data, out["info"].ctypes.data)
    assert st == 0, L.rt_last_error_detail().decode()
    # the signed words as the reference states them
    out["info"] = [int(x) for x in out["info"][:4]] + [int(x) for x in out["info"][4:10].view(np.int32)] + [int(x) for x in out["info"][10:]]
    return out


@pytest.mark.parametrize("name,inputs", CASES, ids=[c[0] for c in CASES])
def test_ranking_matches_reference(gpu, name, inputs):
    """One rt_launch_rank on the case's costs: the order-free assertions, then the 13 words and the returned costs exactly, and the
    part of heavy_pixels the ranking must not write untouched."""
    want = rx.reference_outputs(inputs)
    got = device_rank(gpu, inputs)
    print(name, "device", got["info"], "reference", want["info"])
    rx.check_rank_outputs(inputs, got)
    assert got["info"] == want["info"], dict(zip(rx.INFO_WORDS, zip(got["info"], want["info"])))
    assert np.array_equal(got["cost_out"], want["cost_out"])
    written = int((want["heavy_pixels"] != rx.NO_LIST).sum())     # the listed pixels if the list was sorted, else none
    assert np.all(got["heavy_pixels"][written:] == rx.NO_LIST)
    if written:   # (also where the final rule then dropped the list: heavy_items is 0 and check_rank_outputs did not look)
        listed = got["heavy_pixels"][:written].astype(np.int64)
        assert sorted(listed.tolist()) == sorted(want["heavy_pixels"][:written].tolist())
        p = inputs["params"]
        assert np.all(np.diff(rx.buckets_of(rx.estimates(inputs["cost"], p["nx"], p["smooth_percent"])[listed])) >= 0)


PRIOR_FRAMES = ((96, 64), (100, 37), (300, 200))
PRIOR_GRIDS = ((256, 171), (8, 8))
PRIOR_PARTS = ((None, 0, 1), (4, 0, 2), (4, 1, 2), (8, 2, 3))    # (tile_rows, tile_first, tile_stride); None = the whole frame


@pytest.mark.parametrize("part", PRIOR_PARTS, ids=lambda p: "whole" if p[0] is None else "rows%d-first%d-stride%d" % p)
@pytest.mark.parametrize("grid", PRIOR_GRIDS, ids=lambda g: "cal%dx%d" % g)
@pytest.mark.parametrize("frame", PRIOR_FRAMES, ids=lambda f: "%dx%d" % f)
def test_prior_matches_reference(gpu, frame, grid, part):
    """rt_launch_prior on an asymmetric calibration grid, frames smaller and larger than the grid in either axis, whole and in
    bands: per-pixel costs, tile sums and the total, exactly."""
    nx, ny = frame
    cal_nx, cal_ny = grid
    tile_rows, tile_first, tile_stride = (ny if part[0] is None else part[0]), part[1], part[2]
    cal = rx.calibration_field(cal_nx, cal_ny)
    want_cost, want_tiles, want_total = rx.prior(cal, nx, ny, tile_rows, tile_first, tile_stride)
    rows = rx.local_rows(ny, tile_rows, tile_first, tile_stride)
    assert want_cost.shape == (rows, nx) and rows > 0
    cost = np.zeros((rows, nx), np.uint32)
    tiles = np.zeros(((rows + 7) // 8) * ((nx + 7) // 8), np.uint32)
    total = C.c_uint64(0)
    L = gpu.rt_lib()
    st = L.rt_debug_prior(np.ascontiguousarray(cal).ctypes.data, cal_nx, cal_ny, nx, ny, tile_rows, tile_first, tile_stride, cost.ctypes.data,
                          tiles.ctypes.data, C.byref(total))
    assert st == 0, L.rt_last_error_detail().decode()
    assert np.array_equal(cost, want_cost), np.argwhere(cost != want_cost)[:8]
    assert np.array_equal(tiles, want_tiles)
    assert total.value == want_total


def _cal_cost(gpu, ds):
    L = gpu.rt_lib()
    buf = np.zeros(256 * 256, np.uint32)
    nx, ny = C.c_int32(0), C.c_int32(0)
    st = L.rt_debug_cal_cost(ds._p, buf.ctypes.data, len(buf), C.byref(nx), C.byref(ny))
    assert st == 0, L.rt_last_error_detail().decode()
    return buf[:nx.value * ny.value].reshape(ny.value, nx.value).copy()


def test_calibration_costs_are_the_oracles(gpu, orc):
    """The prior's input: the rays per pixel of the calibration frame (256 pixels wide, 4 spp, seeds 1984 + pixel) that
    rt_scene_create keeps.  Row by row -- row 0 at the bottom, as the oracle's frame -- and in all they are the oracle's ray
    counts, which pins the grid's orientation and contents."""
    nx, ny = 256, 171
    hs = gpu.HostScene("bouncing", nx, ny)
    ds = gpu.DeviceScene(hs)
    try:
        cal = _cal_cost(gpu, ds)
        L = gpu.rt_lib()
        small = np.zeros(64, np.uint32)
        gx, gy = C.c_int32(0), C.c_int32(0)
        assert L.rt_debug_cal_cost(ds._p, small.ctypes.data, 64, C.byref(gx), C.byref(gy)) == 1      # cap below the grid: its size, no data
        assert (gx.value, gy.value) == (nx, ny) and not small.any()
    finally:
        ds.close()
    assert cal.shape == (ny, nx)
    o = orc.OracleScene("bouncing", nx, ny)
    rows = sorted({0, ny - 1} | {(k * (ny - 1)) // 11 for k in range(12)})
    assert len(rows) == 12
    for j in rows:
        assert int(cal[j].sum()) == o.render(4, row0=j, row1=j + 1)[1]["rays"], j
    assert int(cal.sum()) == o.render(4)[1]["rays"]


def _rank_info(gpu, ds):
    L = gpu.rt_lib()
    w = np.zeros(13, np.uint32)
    st = L.rt_debug_rank_info(ds._p, w.ctypes.data)
    return st, dict(zip(rx.INFO_WORDS, (int(x) for x in w))), L.rt_last_error_detail().decode()


def test_shipped_path_ranks_on_the_first_parts_rays(gpu, orc):
    """A default rt_render of `bouncing` 256 x 160 at 32 spp is two parts, [0, 16) and [16, 32); the last ranking is the one before the
    second part and reads the frame's ray counter, to which every kernel of the first part (main, tier, tail) has added and
    nothing else: exactly the oracle's rays of samples [0, 16).  40 960 pixels are 0.16 per resident lane of an MI355X, so
    rank_pixels (rt_abi.hip) takes the lean family's smallest-share row: list from 1.5x, sparse and tier 1 from 2x the mean."""
    nx, ny = 256, 160
    hs = gpu.HostScene("bouncing", nx, ny)
    ds = gpu.DeviceScene(hs)
    try:
        _, stats = ds.render(hs.frame(ns=32))
        st, info, text = _rank_info(gpu, ds)
        assert st == 0, text
        gpu.set_option("prior", 0)
        gpu.set_option("lpt", 0)
        ds.render(hs.frame(ns=32))
        st_off, _, text_off = _rank_info(gpu, ds)
    finally:
        ds.close()
    assert stats.threads_per_group == 512, "bouncing is expected in the lean kernel family (workgroups of 512)"
    rays16 = orc.OracleScene("bouncing", nx, ny).render(16)[1]["rays"]
    p = rx.base_params(nx, ny, "lean_quarter")
    heavy, t1, t2 = rx.thresholds(rays16, nx * ny, (p["heavy_factor"], p["sparse_factor"], p["tier1_factor"]), p["sparse_stride"])
    print("rank info", info, "expected thresholds", heavy, t1, t2, "rays16", rays16)
    assert info["heavy_items"] > 0 and info["heavy_items"] * 2 < nx * ny
    assert (info["heavy_threshold"], info["threshold1"], info["threshold2"]) == (heavy, t1, t2)
    assert info["collected"] == info["heavy_items"] == stats.reserved
    assert st_off == 1 and "not ranked" in text_off
