"""The cost map (include/rt_abi.h, rt_debug_cost_map): the last launches of a ranked frame leave every pixel's ray
count, and the next ranked frame of the same view is ranked on it and runs as one part.  Scheduling only, so every frame here
must equal the CPU oracle bit for bit and count the same rays -- on a cold (two-part) and a warm (one-part) frame, whichever
engine finishes a pixel (main kernel, tier waves, tail launch), whatever map is installed, and across every event that makes
the map stale or drops it.

The smallest ranked frames: 32 samples (2 x split_samples), 64 tiles.  bouncing is the lean spheres-only family with tier 1,
cornell is scanned in lockstep (no tier 1), final is the general family with media.  The general family with tier 1 writes the
map and does not read it (Book-2 final measured slower in one part): its repeat frames stay at two parts, WARM
says so, and everything else is checked on it all the same."""
import ctypes as C

import numpy as np
import pytest

import refit_expect as rf
import reproject_expect as rx

pytestmark = pytest.mark.gpu

NS = 32
CASES = {"bouncing": (256, 160), "cornell": (64, 64), "final": (64, 64)}
# who finishes a pixel: every listed pixel on tier waves; every pixel through the tail launch (the settings of
# test_tail_handoff_matches_oracle); the main kernel and tier 1 alone
ROUTES = {"tiers": {"tier_auto": 0, "heavy_factor_x10": 10, "sparse_factor_x10": 10, "tier1_factor_x10": 10, "tier1_pixels": 65536, "sparse_work_percent": 100},
          "tail": {"handoff_pixels": 1 << 24, "handoff_poll_us": 1, "split_samples": 4, "presplit_samples": 2},
          "no hand-off": {"handoff": 0}}
WARM = {"bouncing": 1, "cornell": 1, "final": 2}      # parts of a frame that finds an exact map
_cache = {}


def _case(art, orc, name):
    """The scene, its frame, the oracle's frame and ray counts (whole frame and row by row); made once."""
    if name not in _cache:
        nx, ny = CASES[name]
        img, iw, ih = art.default_texture(name)
        hs = art.HostScene(name, nx, ny, img, iw, ih)
        o = orc.OracleScene(name, nx, ny, img, iw, ih)
        ref, cnt = o.render(NS)
        rows = np.array([o.render(NS, row0=j, row1=j + 1)[1]["rays"] for j in range(ny)], np.uint64)
        assert int(rows.sum()) == cnt["rays"]
        _cache[name] = dict(hs=hs, orc=o, nx=nx, ny=ny, ref=ref, rays=cnt["rays"], rows=rows, frame=hs.frame(ns=NS))
    return _cache[name]


def _same(got, want, what):
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} values differ, first at {bad[:3].tolist()}"


def _render(ds, c, what, frame=None):
    """One frame that must be the oracle's."""
    fb, st = ds.render(frame or c["frame"])
    assert st.rays == c["rays"], (what, st.rays, c["rays"])
    _same(fb, c["ref"], what)
    return fb, st


@pytest.mark.parametrize("name", list(CASES))
def test_repeat_runs_as_one_part(gpu, orc, name):
    c = _case(gpu, orc, name)
    ds = gpu.DeviceScene(c["hs"])
    try:
        assert ds.cost_map() == ("none", None, 0)
        a, sa = _render(ds, c, f"{name} cold")
        state, cold_map, parts = ds.cost_map()
        assert (state, parts) == ("exact", 2), (state, parts)
        b, sb = _render(ds, c, f"{name} warm")
        state, warm_map, parts = ds.cost_map()
        assert (state, parts) == ("exact", WARM[name]), (state, parts)
        _same(a, b, f"{name} cold against warm")
        assert sa.rays == sb.rays and sa.samples == sb.samples
        assert np.array_equal(cold_map, warm_map)          # a pixel's cost does not depend on who rendered it
    finally:
        ds.close()


@pytest.mark.parametrize("name", list(CASES))
def test_another_seed_equals_a_fresh_scene(gpu, orc, name):
    c = _case(gpu, orc, name)
    other = c["hs"].frame(ns=NS, seed_base=77)
    ref, cnt = c["orc"].render(NS, seed_base=77)
    ds, fresh = gpu.DeviceScene(c["hs"]), gpu.DeviceScene(c["hs"])
    try:
        _render(ds, c, f"{name} first seed")
        got, st = ds.render(other)
        assert ds.cost_map()[0::2] == ("exact", WARM[name])         # the seed is not part of the key
        want, st0 = fresh.render(other)
        assert fresh.cost_map()[2] == 2
        assert st.rays == st0.rays == cnt["rays"]
        _same(got, want, f"{name} seed 77 against a fresh scene")
        _same(got, ref, f"{name} seed 77 against the oracle")
    finally:
        ds.close()
        fresh.close()


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(CASES))
def test_map_holds_every_pixels_rays(gpu, orc, name, route):
    """Row by row the map sums to the oracle's ray count of that row, on a cold and on a warm frame, whoever finishes the pixels:
    the only thing that shows that the main kernel, the tier waves and the tail launch all write the cost."""
    c = _case(gpu, orc, name)
    for k, v in ROUTES[route].items():
        gpu.set_option(k, v)
    L = gpu.rt_lib()
    L.rt_debug_handoff.argtypes = [C.c_void_p, C.c_void_p]
    ds = gpu.DeviceScene(c["hs"])
    try:
        for temp, want_parts in (("cold", None), ("warm", WARM[name] if WARM[name] == 1 else None)):
            _, st = _render(ds, c, f"{name} {route} {temp}")
            state, m, parts = ds.cost_map()
            assert state == "exact" and m.shape == (c["ny"], c["nx"])
            assert parts == want_parts if want_parts else parts >= 2, (temp, parts)
            assert not (m >> 31).any()
            rows = m.sum(axis=1, dtype=np.uint64)
            bad = np.flatnonzero(rows != c["rows"])
            assert len(bad) == 0, f"{name} {route} {temp}: rows {bad[:5].tolist()} sum to {rows[bad[:5]].tolist()}, the oracle counts {c['rows'][bad[:5]].tolist()}"
            assert int(rows.sum()) == st.rays
            # the route did run
            info, handed = np.zeros(13, np.uint32), np.zeros(2, np.uint64)
            assert L.rt_debug_rank_info(ds._p, info.ctypes.data) == 0 and L.rt_debug_handoff(ds._p, handed.ctypes.data) == 0
            if route == "tiers" and name != "cornell":
                assert info[2] > 0 and info[2] == info[0], info.tolist()      # tier 1 holds the whole list
            if route == "tail":
                assert handed[0] > 0
            if route == "no hand-off":
                assert handed[0] == 0
    finally:
        ds.close()


@pytest.mark.parametrize("name", list(CASES))
def test_any_installed_map_leaves_the_frame_alone(gpu, orc, name):
    c = _case(gpu, orc, name)
    n = c["nx"] * c["ny"]
    ds = gpu.DeviceScene(c["hs"])
    try:
        with pytest.raises(gpu.RtError, match="no ranked frame"):
            ds.set_cost_map(np.ones(n, np.uint32))
        _render(ds, c, f"{name} cold")
        true = ds.cost_map()[1].ravel()
        with pytest.raises(gpu.RtError, match="pixel count"):
            ds.set_cost_map(true[:-1])
        one = np.zeros(n, np.uint32)
        one[n // 3] = 2 ** 31 - 1
        w = WARM[name]
        maps = {"zeros": (np.zeros(n, np.uint32), 2), "equal": (np.full(n, 1000, np.uint32), w), "reversed": (true[::-1], w),
                "random": (np.random.default_rng(3).integers(0, 2 ** 31, n, dtype=np.uint32), w), "one pixel": (one, w),
                "flagged": (true | np.uint32(0x80000000), w)}
        for tag, (m, want_parts) in maps.items():
            ds.set_cost_map(m)
            state, got, _ = ds.cost_map()
            assert state == "exact" and np.array_equal(got.ravel(), m & np.uint32(0x7FFFFFFF)), tag
            _render(ds, c, f"{name} map {tag}")
            state, got, parts = ds.cost_map()
            assert (state, parts) == ("exact", want_parts), (tag, state, parts)     # a map that sums to 0 is not used
            assert np.array_equal(got.ravel(), true), tag                          # ... and the frame left the true one
    finally:
        ds.close()


def _shifted(cam):
    """The camera moved a little sideways and up, its frame with it."""
    out = type(cam).from_buffer_copy(cam)
    for k, d in enumerate((0.05, 0.03, -0.04)):
        out.origin[k] += d
        out.lower_left_corner[k] += d
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_what_makes_the_map_stale_or_drops_it(gpu, orc, name):
    c = _case(gpu, orc, name)
    nx, ny = c["nx"], c["ny"]
    cam0 = c["hs"].desc.camera
    cam1 = _shifted(cam0)
    moved = rx.WithCamera(gpu, c["hs"], cam1)
    ds, fresh = gpu.DeviceScene(c["hs"]), gpu.DeviceScene(moved)
    try:
        want1, st1 = fresh.render(c["frame"])
        assert not np.array_equal(want1, c["ref"])
        _render(ds, c, "cold")
        _render(ds, c, "warm")
        assert ds.cost_map()[0::2] == ("exact", WARM[name])
        # an option call, even one that changes nothing: stale, two parts, then exact again
        gpu.set_option("tier_priority", 1)
        assert ds.cost_map()[0] == "stale"
        _render(ds, c, "after set_option")
        assert ds.cost_map()[0::2] == ("exact", 2)
        _render(ds, c, "warm again")
        assert ds.cost_map()[0::2] == ("exact", WARM[name])
        # the camera moved, the prior kept: the map is that prior
        ds.set_camera(cam1)
        assert ds.cost_map()[0] == "stale"
        got, st = ds.render(c["frame"])
        assert ds.cost_map()[0::2] == ("exact", 2) and st.rays == st1.rays
        _same(got, want1, "moved camera, stale map")
        got, st = ds.render(c["frame"])
        assert ds.cost_map()[0::2] == ("exact", WARM[name]) and st.rays == st1.rays
        _same(got, want1, "moved camera, warm")
        # ... and back with a recalibration: no map
        ds.set_camera(cam0, recalibrate=True)
        assert ds.cost_map()[0] == "none"
        _render(ds, c, "camera back, recalibrated")
        assert ds.cost_map()[0::2] == ("exact", 2)
        # another partition of the same pixels, another width: no reuse, and the map is then theirs
        for kw in (dict(tile_rows=ny // 2), dict(nx=nx + 8, ny=ny)):
            f = c["hs"].frame(ns=NS, **kw)
            got, st = ds.render(f)
            state, m, parts = ds.cost_map()
            assert (state, parts, m.shape) == ("exact", 2, (ny, f.nx)), (kw, state, parts, m.shape)
            again, st2 = ds.render(f)
            assert ds.cost_map()[0::2] == ("exact", WARM[name]) and st.rays == st2.rays
            _same(again, got, f"{kw} warm against cold")
        other = gpu.DeviceScene(c["hs"])
        try:
            want, st0 = other.render(f)
        finally:
            other.close()
        assert st0.rays == st.rays
        _same(got, want, "another width against a fresh scene")
        _render(ds, c, "the first geometry again")
        assert ds.cost_map()[0::2] == ("exact", 2)
        # unranked frames neither read nor write the map
        _, before, _ = ds.cost_map()
        gpu.set_option("lpt", 0)
        _render(ds, c, "lpt 0")
        gpu.reset_options()
        ds.render(c["hs"].frame(ns=NS // 2))
        state, after, parts = ds.cost_map()
        assert (state, parts) == ("stale", 2) and np.array_equal(before, after)
        # cost_map 0: the map is neither used nor written nor shown
        gpu.set_option("cost_map", 0)
        for k in range(2):
            _render(ds, c, f"cost_map 0, frame {k}")
            assert ds.cost_map() == ("none", None, 2)
        with pytest.raises(gpu.RtError, match="cost_map is 0"):
            ds.set_cost_map(before)
        gpu.set_option("cost_map", 1)
        assert ds.cost_map()[0] == "stale" and np.array_equal(ds.cost_map()[1], before)
    finally:
        ds.close()
        fresh.close()


def test_shares_of_a_frame_have_maps_of_their_own(gpu, orc):
    """tile_first and tile_stride are part of the key, and the map is addressed by LOCAL rows: after a whole-frame map the first
    frame of a share (every other band of 8 rows: what one rank of two renders) is two parts, its repeat one, the other rank's
    share two again, and so on for one rank of three (7 bands, 56 rows).  Every frame is the oracle's rows of that share and a
    fresh scene's frame bit for bit, and the share's map sums row by row to the oracle's counts of its global rows."""
    c = _case(gpu, orc, "bouncing")
    ds = gpu.DeviceScene(c["hs"])
    try:
        _render(ds, c, "whole frame")
        assert ds.cost_map()[0::2] == ("exact", 2)
        for first, stride in ((0, 2), (1, 2), (1, 3)):
            f = c["hs"].frame(ns=NS, tile_rows=8, tile_first=first, tile_stride=stride)
            rows = gpu.local_rows_to_global(f)
            assert 0 < len(rows) < c["ny"] and (len(rows) // 8) * (c["nx"] // 8) >= 64
            fresh = gpu.DeviceScene(c["hs"])
            try:
                want, st0 = fresh.render(f)
            finally:
                fresh.close()
            _same(want, c["ref"][rows], f"share {first}/{stride}, fresh scene against the oracle")
            assert st0.rays == int(c["rows"][rows].sum())
            for want_parts in (2, 1):
                what = f"share {first}/{stride}, {want_parts} part(s)"
                got, st = ds.render(f)
                state, m, parts = ds.cost_map()
                assert (state, parts, m.shape) == ("exact", want_parts, (len(rows), c["nx"])), (what, state, parts, m.shape)
                assert st.rays == st0.rays and st.local_rows == len(rows), what
                _same(got, want, what)
                sums = m.sum(axis=1, dtype=np.uint64)
                bad = np.flatnonzero(sums != c["rows"][rows])
                assert len(bad) == 0, f"{what}: local rows {bad[:5].tolist()} sum to {sums[bad[:5]].tolist()}, the oracle counts {c['rows'][rows][bad[:5]].tolist()}"
        _render(ds, c, "the whole frame again")
        assert ds.cost_map()[0::2] == ("exact", 2)
    finally:
        ds.close()


def test_unranked_frames_leave_no_map(gpu, orc):
    c = _case(gpu, orc, "cornell")
    ds = gpu.DeviceScene(c["hs"])
    try:
        ds.render(c["hs"].frame(ns=NS // 2))
        assert ds.cost_map() == ("none", None, 0)
        gpu.set_option("lpt", 0)
        _render(ds, c, "lpt 0")
        assert ds.cost_map() == ("none", None, 0)
    finally:
        ds.close()


@pytest.mark.parametrize("recalibrate", [False, True])
def test_moved_spheres(gpu, orc, recalibrate):
    c = _case(gpu, orc, "bouncing")
    idx, rec = rf.make_update(c["hs"], "all")
    moved = rf.moved_scene(c["hs"], idx, rec)
    ref, cnt = orc.OracleScene.from_host(moved, c["nx"], c["ny"]).render(NS)
    ds = gpu.DeviceScene(c["hs"])
    try:
        _render(ds, c, "cold")
        ds.update_spheres(rec, idx, recalibrate=recalibrate)
        assert ds.cost_map()[0] == ("none" if recalibrate else "stale")
        got, st = ds.render(c["frame"])
        assert ds.cost_map()[0::2] == ("exact", 2) and st.rays == cnt["rays"]
        _same(got, ref, f"moved spheres, recalibrate={recalibrate}")
        got, st = ds.render(c["frame"])
        assert ds.cost_map()[0::2] == ("exact", 1) and st.rays == cnt["rays"]
        _same(got, ref, "moved spheres, warm")
    finally:
        ds.close()


def test_non_blocking_frames_back_to_back(gpu, orc):
    """Two non-blocking renders into device memory on one stream with rt_frame_finish between them, as the benchmark's steps are:
    the map counts from the finish on, so the second frame is one part."""
    import torch
    c = _case(gpu, orc, "bouncing")
    buf = torch.zeros((c["ny"], c["nx"], 3), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    ds = gpu.DeviceScene(c["hs"])
    try:
        frames = []
        for want_parts in (2, 1):
            ds.render(c["frame"], out=buf.data_ptr(), stream=stream, blocking=False)
            st = ds.finish()
            assert st.rays == c["rays"]
            assert ds.cost_map()[0::2] == ("exact", want_parts)
            frames.append(buf.cpu().numpy())
            buf.zero_()
        _same(frames[0], c["ref"], "first non-blocking frame")
        _same(frames[1], c["ref"], "second non-blocking frame")
    finally:
        ds.close()
