"""rt_render_aov / DeviceScene.render_aov on the GPU: every buffer against the CPU oracle (tests/aov_expect.py: the emissive
twin's render and the oracle's trace of the twin's ray sample), the twin identity against rt_render itself, the ids against
rt_trace_rays, frame shapes around a wave, a tile and a workgroup, the empty world, the row partition, the option, output
subsets, the torch path and a call beside a pending render.  Every comparison is bit for bit: no tolerance anywhere."""

import numpy as np
import pytest

import aov_expect as ax
import scene_gen as sg

pytestmark = pytest.mark.gpu

FLOATS = ("albedo", "normal", "depth", "alpha")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def cases(gpu, orc):
    """(Case, DeviceScene) by scene; computed once, left unchanged."""
    cache = {}

    def get(key):
        if key not in cache:
            c = ax.Case(gpu, orc, key)
            cache[key] = (c, gpu.DeviceScene(c.scene))
        return cache[key]
    yield get
    for _, ds in cache.values():
        ds.close()


def _frame(c, ns, nx=ax.NX, ny=ax.NY, **kw):
    return c.scene.frame(nx=nx, ny=ny, ns=ns, seed_base=ax.SEED, **kw)


def _assert_same(got, want, names, what, rows=slice(None)):
    for k in names:
        g, w = got[k], want[k][rows]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype)
        bad = np.argwhere(_bits(g) != _bits(w))
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} of {g.size} values, first at {bad[:3].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("key", ax.PARITY)
def test_aov_matches_oracle(cases, key, ns):
    """All four float buffers and mat, ns = 1 and 3 (an inexact scale factor, and a chain carried across samples)."""
    c, ds = cases(key)
    got = ds.render_aov(_frame(c, ns), ids=True)
    assert set(got) == set(FLOATS) | {"prim", "inst", "mat"}
    _assert_same(got, c.expect(ns), FLOATS + ("mat",), f"{key} ns={ns}")
    assert ((got["prim"] >= 0) == (got["mat"] >= 0)).all() and (got["inst"] >= -1).all()


@pytest.mark.parametrize("gradient", [0, 1])
@pytest.mark.parametrize("seed", [ax.SEED, 77_000_000_019])
@pytest.mark.parametrize("key", [ax.SPHERES, ax.GENERAL])
def test_albedo_is_rt_render_of_the_twin(gpu, cases, key, seed, gradient):
    """The identity on the device: rt_render of the emissive twin at gamma 1, same ns, seed, background and gradient."""
    c, ds = cases(key)
    f = c.scene.frame(nx=ax.NX, ny=ax.NY, ns=3, gamma=1.0, seed_base=seed)
    f.use_gradient_bg = gradient
    lit = gpu.DeviceScene(c.twin)
    try:
        fb, st = lit.render(f)
    finally:
        lit.close()
    assert st.rays == ax.NX * ax.NY * 3          # no path of the twin goes on
    f.gamma = 2.2                                # ignored by the feature pass
    _assert_same(ds.render_aov(f, normal=False, depth=False, alpha=False), {"albedo": fb}, ("albedo",), f"{key} seed={seed} gradient={gradient}")


@pytest.mark.parametrize("key", [ax.SPHERES, ax.GENERAL, ax.PARITY[5]])
def test_ids_are_rt_trace_rays_on_the_first_primary_rays(cases, key):
    """prim, inst and mat equal DeviceScene.trace(record=True) on the ns = 1 ray sample; so does depth, as t."""
    c, ds = cases(key)
    rays = c.expect(1)["rays"]
    r = ds.trace(np.ascontiguousarray(rays[:, 0:3]), np.ascontiguousarray(rays[:, 3:6]), np.ascontiguousarray(rays[:, 6]), record=True)
    got = ds.render_aov(_frame(c, 1), albedo=False, normal=False, alpha=False, ids=True)
    for k, w in (("prim", r.prim), ("inst", r.inst), ("mat", r.mat)):
        assert np.array_equal(got[k], w.reshape(ax.NY, ax.NX)), k
    hit = r.prim >= 0
    assert np.array_equal(_bits(got["depth"]), _bits(np.where(hit, r.t, np.float32(0)).reshape(ax.NY, ax.NX)))
    assert hit.any() and (~hit).any()
    if key == ax.GENERAL:
        assert (got["inst"] >= 0).any() and len(np.unique(gpu_kind(got["prim"][got["prim"] >= 0]))) >= 2


def gpu_kind(ref):
    return (np.asarray(ref).astype(np.int64) & 0xFFFFFFFF) >> 28


@pytest.mark.parametrize("nx,ny", [(63, 1), (8, 8), (13, 5), (257, 1), (50, 35)])
@pytest.mark.parametrize("key", [ax.SPHERES, ax.GENERAL])
def test_frame_shapes(cases, key, nx, ny):
    """63, 64, 65 and 257 pixels -- a wave, a tile, a workgroup and one more -- as rows and as blocks, and 50 x 35: tiles that
    overhang the right and the top edge.  The scene's camera is unchanged, so the frames are stretched; the oracle's are too."""
    c, ds = cases(key)
    got = ds.render_aov(_frame(c, 3, nx, ny), ids=True)
    _assert_same(got, c.expect(3, nx, ny), FLOATS + ("mat",), f"{key} {nx}x{ny}")


def test_empty_world(gpu, orc):
    """n_nodes = 0: every sample misses; albedo is the miss term -- the oracle's frame of the empty twin, and with a constant
    background and one sample the background itself."""
    scene = sg.generate("spheres_plain", 1, ax.NX, ax.NY).emptied()
    assert scene.desc.n_nodes == 0
    ds = gpu.DeviceScene(scene)
    try:
        f = scene.frame(nx=ax.NX, ny=ax.NY, ns=3, seed_base=ax.SEED)
        got = ds.render_aov(f, ids=True)
        want = ax.expected(orc, scene, ax.NX, ax.NY, 3, gpu)
        assert (want["mat"] == -1).all()
        _assert_same(got, want, FLOATS + ("mat",), "empty world")
        for k in ("normal", "depth", "alpha"):
            assert (_bits(got[k]) == 0).all(), k
        assert (got["prim"] == -1).all() and (got["inst"] == -1).all()
        f.ns, f.use_gradient_bg = 1, 0
        flat = ds.render_aov(f, normal=False, depth=False, alpha=False)["albedo"]
        assert np.array_equal(_bits(flat), _bits(np.broadcast_to(np.array(scene.background, np.float32), flat.shape)))
    finally:
        ds.close()


def test_row_partition(gpu, cases):
    """tile_rows = 4, tile_first = 1, tile_stride = 3: those rows of the whole frame, in compact local rows."""
    c, ds = cases(ax.GENERAL)
    f = _frame(c, 3, tile_rows=4, tile_first=1, tile_stride=3)
    rows = gpu.local_rows_to_global(f)
    assert list(rows) == [4, 5, 6, 7, 16, 17, 18, 19, 28, 29, 30, 31]
    got = ds.render_aov(f, ids=True)
    _assert_same(got, c.expect(3), FLOATS + ("mat",), "partition", rows)
    whole = ds.render_aov(_frame(c, 3), ids=True)
    _assert_same(got, whole, ("prim", "inst"), "partition", rows)


@pytest.mark.parametrize("key", [ax.PARITY[0], ax.GENERAL])
def test_every_option_gives_the_same_buffers(gpu, cases, key):
    """aov_lds -1, 0, 1 and 2 on a spheres-only and on a general scene."""
    c, ds = cases(key)
    want = c.expect(3)
    ref = None
    try:
        for lds in (-1, 0, 1, 2):
            gpu.set_option("aov_lds", lds)
            got = ds.render_aov(_frame(c, 3), ids=True)
            _assert_same(got, want, FLOATS + ("mat",), f"{key} aov_lds={lds}")
            ref = ref or got
            _assert_same(got, ref, ("prim", "inst"), f"{key} aov_lds={lds}")
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("key", [ax.SPHERES, ax.GENERAL])
def test_output_subsets(cases, key):
    """Each output alone -- the kernel then skips what the others would need -- equals the same output among all of them."""
    c, ds = cases(key)
    want = c.expect(3)
    f = _frame(c, 3)
    every = ds.render_aov(f, ids=True)
    only = ds.render_aov(f, albedo=False, normal=False, alpha=False)
    assert set(only) == {"depth"}
    _assert_same(only, want, ("depth",), f"{key} depth only")
    for k in every:
        one = ds.render_aov(f, out={k: np.empty_like(every[k])})
        assert np.array_equal(one[k].view(np.uint32), every[k].view(np.uint32)), k


def test_torch_tensors_on_a_side_stream(cases):
    """out = torch device tensors: written in place, enqueued on the given stream, not waited for with blocking=False."""
    import torch
    c, ds = cases(ax.GENERAL)
    want = c.expect(3)
    f = _frame(c, 3)
    dev = torch.device("cuda", ds.device)
    out = {k: torch.full((ax.NY, ax.NX, 3) if k in ("albedo", "normal") else (ax.NY, ax.NX), -7,
                         dtype=torch.float32 if k in FLOATS else torch.int32, device=dev) for k in FLOATS + ("mat",)}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ret = ds.render_aov(f, out=out, stream=s, blocking=False)
    s.synchronize()
    assert ret is out
    _assert_same({k: v.cpu().numpy() for k, v in out.items()}, want, FLOATS + ("mat",), "torch, side stream")
    again = {"depth": torch.zeros((ax.NY, ax.NX), dtype=torch.float32, device=dev)}
    torch.cuda.synchronize()
    ds.render_aov(f, out=again, stream=s.cuda_stream)          # an integer stream handle, blocking
    assert np.array_equal(_bits(again["depth"].cpu().numpy()), _bits(want["depth"]))
    with pytest.raises(ValueError):
        ds.render_aov(f, out={"depth": torch.zeros((ax.NY, ax.NX), dtype=torch.float32)})               # a CPU tensor
    with pytest.raises(ValueError):
        ds.render_aov(f, out={"depth": again["depth"], "alpha": np.zeros((ax.NY, ax.NX), np.float32)})   # mixed


def test_aov_beside_a_pending_render(cases):
    """A non-blocking render of the scene on one stream and a feature pass on another: both give their standalone results
    (test_trace_beside_a_pending_render)."""
    import torch
    c, ds = cases("bouncing")
    want = c.expect(3)
    frame = c.scene.frame(nx=ax.NX, ny=ax.NY, ns=64)
    ref_fb, ref_st = ds.render(frame)
    dev = torch.device("cuda", ds.device)
    buf = torch.zeros((ax.NY, ax.NX, 3), dtype=torch.float32, device=dev)
    out = {k: torch.zeros((ax.NY, ax.NX, 3) if k in ("albedo", "normal") else (ax.NY, ax.NX), dtype=torch.float32, device=dev) for k in FLOATS}
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ds.render(frame, out=buf.data_ptr(), stream=sa.cuda_stream, blocking=False)
    ds.render_aov(_frame(c, 3), out=out, stream=sb, blocking=False)
    sb.synchronize()
    st = ds.finish()
    sa.synchronize()
    assert st.rays == ref_st.rays
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(ref_fb))
    _assert_same({k: v.cpu().numpy() for k, v in out.items()}, want, FLOATS, "beside a render")
