"""rt_radiance_rays / DeviceScene.radiance on the GPU: per-query parity with the CPU oracle (tests/radiance_expect.py: a query
is a 1 x 1 frame of a degenerate camera), the option, the same identity against rt_render itself, batch shapes, the torch
path, edge rays, and a query beside a pending render.  Every comparison is bit-identical colours and equal ray counts."""

import numpy as np
import pytest

import radiance_expect as rx

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def cases(gpu, orc):
    """(Case, DeviceScene) by scene; computed once, left unchanged."""
    cache = {}

    def get(key, n):
        if (key, n) not in cache:
            c = rx.Case(gpu, orc, key, n)
            cache[(key, n)] = (c, gpu.DeviceScene(c.scene))
        return cache[(key, n)]
    yield get
    for _, ds in cache.values():
        ds.close()


def _query(c, ds, kind, ns, sel=slice(None), **kw):
    seeds = None if kind == "default" else c.seeds(kind)[sel]
    return ds.radiance(c.o[sel], c.d[sel], c.tm[sel], ns=ns, seeds=seeds, count_rays=True, **kw)


def _assert_same(r, rgb, rays, what):
    bad = np.flatnonzero((_bits(r.rgb) != _bits(rgb)).any(1) | (r.rays != rays))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(rgb)} queries differ, first {bad[:5]}: {r.rgb[bad[:3]]} vs {rgb[bad[:3]]}, rays {r.rays[bad[:5]]} vs {rays[bad[:5]]}"


@pytest.mark.parametrize("seeding", ["default", "explicit"])
@pytest.mark.parametrize("ns", [1, 4])
@pytest.mark.parametrize("key,n", rx.PARITY)
def test_radiance_matches_oracle_per_query(cases, key, n, ns, seeding):
    """Case 1: colour bit for bit and the ray count of every query, default seeds (seed_base + i) and explicit ones."""
    c, ds = cases(key, n)
    rgb, rays = c.expect(seeding, ns)
    _assert_same(_query(c, ds, seeding, ns), rgb, rays, f"{key} ns={ns} {seeding} seeds")


@pytest.mark.parametrize("key", [rx.PARITY[0][0], rx.PARITY[4][0]])
def test_every_option_gives_the_same_answer(gpu, cases, key):
    """Case 2: radiance_lds -1, 0, 1 and 2 on a spheres-only and on a general scene."""
    c, ds = cases(key, 2048)
    rgb, rays = c.expect("explicit", 4)
    try:
        for lds in (-1, 0, 1, 2):
            gpu.set_option("radiance_lds", lds)
            _assert_same(_query(c, ds, "explicit", 4), rgb, rays, f"{key} radiance_lds={lds}")
    finally:
        gpu.reset_options()


def test_query_is_a_pixel_of_rt_render(gpu, cases):
    """Case 3: the identity itself, on the device: a scene whose description carries the degenerate camera, rendered 1 x 1 at
    8 spp and gamma 1 with seed_base = the query's seed, gives the query's colour and ray count."""
    c, ds = cases(rx.PARITY[4][0], 2048)
    sel = np.array([5, 900, 1800])           # one query of each third of the ray set
    seeds = c.seeds("explicit")[sel]
    r = ds.radiance(c.o[sel], c.d[sel], c.tm[sel], ns=8, seeds=seeds, count_rays=True)

    class Degenerate:
        pass
    for k, i in enumerate(sel):
        g = Degenerate()
        g.desc = rx.degenerate_desc(c.scene, c.o[i], c.p[i], c.tm[i])
        f = c.scene.frame(nx=1, ny=1, ns=8, gamma=1.0, seed_base=int(seeds[k]))
        one = gpu.DeviceScene(g)
        try:
            fb, st = one.render(f)
        finally:
            one.close()
        assert np.array_equal(_bits(fb[0, 0]), _bits(r.rgb[k])), (i, fb[0, 0], r.rgb[k])
        assert st.rays == r.rays[k]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_sizes(cases, n):
    """Case 4a: batches around a wave and a workgroup, against the oracle; the empty batch gives empty outputs."""
    c, ds = cases(rx.PARITY[0][0], 2048)
    rgb, rays = c.expect("explicit", 4)
    sel = slice(1000, 1000 + n)
    r = _query(c, ds, "explicit", 4, sel)
    assert r.rgb.shape == (n, 3) and r.rays.shape == (n,)
    _assert_same(r, rgb[sel], rays[sel], f"n={n}")
    if n == 0:
        assert ds.radiance(c.o[sel], c.d[sel]).rays is None


def test_batch_larger_than_the_resident_lanes(cases):
    """Case 4b: 600 000 queries -- more than the lanes resident at once, so every lane strides and refills -- made of 4096
    oracle-checked queries tiled with their explicit seeds: every repeat equals the first block bit for bit."""
    import torch
    c, ds = cases(*rx.LARGE)
    rgb, rays = c.expect("explicit", 1)
    n, m = 600_000, c.n
    reps = -(-n // m)
    tile = lambda x: torch.from_numpy(np.concatenate([x] * reps)[:n]).cuda()   # noqa: E731
    r = ds.radiance(tile(c.o), tile(c.d), tile(c.tm), ns=1, seeds=tile(c.seeds("explicit").view(np.int64)), count_rays=True)
    torch.cuda.synchronize()
    got_rgb, got_rays = r.rgb.cpu().numpy(), r.rays.cpu().numpy()
    assert np.array_equal(_bits(got_rgb[:m]), _bits(rgb)) and np.array_equal(got_rays[:m], rays)
    assert np.array_equal(_bits(got_rgb), _bits(np.concatenate([rgb] * reps)[:n]))
    assert np.array_equal(got_rays, np.concatenate([rays] * reps)[:n])


def test_torch_path(cases):
    """Case 5: device tensors in place on the current and on a side stream, non-contiguous inputs, outputs on the device, int64
    and uint64 seeds, and the numpy path gives the same."""
    import torch
    c, ds = cases(rx.PARITY[4][0], 2048)
    rgb, rays = c.expect("explicit", 4)
    seeds = c.seeds("explicit")
    ref = ds.radiance(c.o, c.d, c.tm, ns=4, seeds=seeds, count_rays=True)
    ref_i64 = ds.radiance(c.o, c.d, c.tm, ns=4, seeds=seeds.view(np.int64), count_rays=True)
    assert isinstance(ref.rgb, np.ndarray) and ref.rays.dtype == np.int32
    _assert_same(ref, rgb, rays, "numpy path")
    _assert_same(ref_i64, rgb, rays, "numpy path, int64 seeds")
    ot, dt, tt = (torch.from_numpy(x).cuda() for x in (c.o, c.d, c.tm))
    st = torch.from_numpy(seeds.view(np.int64)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        r1 = ds.radiance(ot, dt, tt, ns=4, seeds=st, count_rays=True)
    r2 = ds.radiance(ot, dt, tt, ns=4, seeds=st, count_rays=True, stream=s)
    s.synchronize()
    wide = torch.cat([ot, dt], 1)                      # (N, 6): its column slices are not contiguous
    assert not wide[:, 0:3].is_contiguous()
    r3 = ds.radiance(wide[:, 0:3], wide[:, 3:6], tt, ns=4, seeds=st, count_rays=True)
    torch.cuda.synchronize()
    for r in (r1, r2, r3):
        assert all(isinstance(x, torch.Tensor) and x.device == ot.device for x in r)
        assert r.rgb.dtype == torch.float32 and r.rays.dtype == torch.int32
        assert np.array_equal(_bits(r.rgb.cpu().numpy()), _bits(rgb)) and np.array_equal(r.rays.cpu().numpy(), rays)
    with pytest.raises(ValueError):
        ds.radiance(ot, dt, tt, seeds=st.int())
    with pytest.raises(ValueError):
        ds.radiance(ot, c.d, tt)


def test_side_stream_waits_for_the_current_stream(cases):
    """stream= other than the current one: the inputs' contiguous copies and the outputs are made on the current stream, so
    the query must not start before that stream's pending work (test_trace_rays.py, the same arrangement): the blocks the
    copies reuse hold NaN until the work behind the sleep overwrites them, and a NaN ray would give zeros."""
    import torch
    c, ds = cases(rx.PARITY[0][0], 2048)
    rgb, rays = c.expect("default", 1)
    ot, dt, tt = (torch.from_numpy(x).cuda() for x in (c.o, c.d, c.tm))
    n = c.n
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    junk = [torch.full((n, 6), float("nan"), device="cuda"), torch.full((n, 3), float("nan"), device="cuda"),
            torch.full((n, 3), float("nan"), device="cuda")]
    del junk                                           # back to the cache of the current stream, NaN inside
    torch.cuda._sleep(50_000_000)                      # the current stream is busy for a while
    wide = torch.cat([ot, dt], 1)                      # written after the sleep
    r = ds.radiance(wide[:, 0:3], wide[:, 3:6], tt, ns=1, count_rays=True, stream=s)
    s.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(r.rgb.cpu().numpy()), _bits(rgb)) and np.array_equal(r.rays.cpu().numpy(), rays)


@pytest.mark.parametrize("key", [rx.PARITY[0][0], rx.PARITY[4][0], "cornell_smoke"])
def test_edge_rays(cases, key):
    """Case 6: a NaN or infinite component in the origin, direction or time, and the zero direction, give zeros and 0 rays;
    with explicit seeds every other query of the batch is unchanged."""
    c, ds = cases(key, 1024 if key == "cornell_smoke" else 2048)
    rgb, rays = c.expect("explicit", 4)
    o, d, tm = c.o.copy(), c.d.copy(), c.tm.copy()
    bad = np.arange(0, c.n, 7)
    for k, i in enumerate(bad):
        what = k % 8
        v = [np.nan, np.inf, -np.inf][k % 3]
        if what < 3:
            o[i, what] = v
        elif what < 6:
            d[i, what - 3] = v
        elif what == 6:
            tm[i] = v
        else:
            d[i] = [0.0, -0.0, 0.0]
    r = ds.radiance(o, d, tm, ns=4, seeds=c.seeds("explicit"), count_rays=True)
    good = np.ones(c.n, bool)
    good[bad] = False
    assert (_bits(r.rgb[bad]) == 0).all() and (r.rays[bad] == 0).all()
    assert np.array_equal(_bits(r.rgb[good]), _bits(rgb[good])) and np.array_equal(r.rays[good], rays[good])
    only_bad = ds.radiance(o[bad], d[bad], tm[bad], ns=4, count_rays=True)      # a batch with nothing to walk
    assert (_bits(only_bad.rgb) == 0).all() and (only_bad.rays == 0).all()


def test_radiance_beside_a_pending_render(gpu, cases):
    """Case 7: a non-blocking render of the scene on one stream and a query batch on another: both give their standalone
    results (test_trace_beside_a_pending_render)."""
    import torch
    c, ds = cases("bouncing", 2048)
    rgb, rays = c.expect("default", 4)
    frame = c.scene.frame(nx=rx.NX, ny=rx.NY, ns=64)
    ref_fb, ref_st = ds.render(frame)
    ot, dt, tt = (torch.from_numpy(x).cuda() for x in (c.o, c.d, c.tm))
    buf = torch.zeros((rx.NY, rx.NX, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ds.render(frame, out=buf.data_ptr(), stream=sa.cuda_stream, blocking=False)
    r = ds.radiance(ot, dt, tt, ns=4, count_rays=True, stream=sb)
    sb.synchronize()
    st = ds.finish()
    sa.synchronize()
    assert st.rays == ref_st.rays
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(ref_fb))
    assert np.array_equal(_bits(r.rgb.cpu().numpy()), _bits(rgb)) and np.array_equal(r.rays.cpu().numpy(), rays)
