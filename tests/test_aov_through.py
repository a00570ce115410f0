"""rt_render_aov_through / DeviceScene.render_aov_through on the GPU: every output against tests/aov_through_expect.py (the
oracle's walks and a NumPy float32 restatement of the chain's arithmetic), max_bounces = 0 and a fuzz limit below every fuzz
against rt_render_aov itself, the ids against rt_trace_rays on the chains' last rays, a ragged frame, a row share, the option,
output subsets, the torch path, rt_render before and after, and the command line.  Every comparison is bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import aov_expect as ax
import aov_through_expect as tx

pytestmark = pytest.mark.gpu

FLOATS = ("albedo", "normal", "depth", "alpha", "through")
CHECKED = FLOATS + ("mat", "bounces")
EVERY = dict(ids=True, through=True, bounces=True)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def world(gpu, orc):
    """The expectations (tx.Cases, with the twins' device scenes behind them) and the device scenes, by scene key; made once."""
    scenes, twins = {}, {}

    def twin(key):
        if key not in twins:
            twins[key] = gpu.DeviceScene(cases.case(key).twin)
        return twins[key]
    cases = tx.Cases(gpu, orc, twin)

    def scene(key):
        if key not in scenes:
            scenes[key] = gpu.DeviceScene(cases.case(key).scene)
        return scenes[key]
    yield cases, scene
    for ds in list(scenes.values()) + list(twins.values()):
        ds.close()


def _frame(cases, key, ns, nx=ax.NX, ny=ax.NY, **kw):
    return cases.case(key).scene.frame(nx=nx, ny=ny, ns=ns, seed_base=ax.SEED, **kw)


def _assert_same(got, want, names, what, rows=slice(None)):
    for k in names:
        g, w = got[k], want[k][rows]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(_bits(g) != _bits(w))
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} of {g.size} values, first at {bad[:3].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"


def _assert_ids(ds, got, e, what):
    """prim and inst are rt_trace_rays' on the last ray of sample 0's chain (a terminal miss gives -1 there too)."""
    c = e["chain"]
    o, d, tm = (np.ascontiguousarray(c[k][:, :, 0].reshape(-1, *c[k].shape[3:])) for k in ("last_o", "last_d", "last_tm"))
    r = ds.trace(o, d, tm, record=True)
    for k, w in (("prim", r.prim), ("inst", r.inst), ("mat", r.mat)):
        assert np.array_equal(got[k], w.reshape(got[k].shape)), (what, k)


MATCH = [(key, f, mb) for key in (tx.SPHERES, tx.GENERAL) for f in tx.FRAMES for mb in tx.BOUNCES] + \
        [(tx.GENERAL2, tx.FRAMES[1], mb) for mb in tx.BOUNCES]


@pytest.mark.parametrize("key,frame,mb", MATCH, ids=[f"{k}-{f[0]}x{f[1]}@{f[2]}-mb{mb}" for k, f, mb in MATCH])
def test_through_matches_expectation(world, key, frame, mb):
    """Every output on a spheres-only scene with glass and metals and on two general scenes, at 48 x 32 with 1 and 4 samples
    and on a ragged 13 x 9 frame (tiles overhang both edges), max_bounces 1, 2 and 8."""
    cases, scene = world
    nx, ny, ns = frame
    ds = scene(key)
    got = ds.render_aov_through(_frame(cases, key, ns, nx, ny), mb, tx.FUZZ_LIMIT, **EVERY)
    assert set(got) == set(CHECKED) | {"prim", "inst"}
    e = cases.expect(key, nx, ny, ns, mb)
    assert not np.isnan(e["albedo"]).any()
    _assert_same(got, e, CHECKED, f"{key} {frame} max_bounces={mb}")
    _assert_ids(ds, got, e, f"{key} {frame} max_bounces={mb}")


@pytest.mark.parametrize("key", [tx.SPHERES, tx.GENERAL])
def test_row_share(gpu, world, key):
    """tile_rows = 4, tile_first = 1, tile_stride = 2: those rows of the whole frame, in compact local rows."""
    cases, scene = world
    f = _frame(cases, key, 4, **tx.SHARE)
    rows = gpu.local_rows_to_global(f)
    assert list(rows) == [4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23, 28, 29, 30, 31]
    got = scene(key).render_aov_through(f, 8, tx.FUZZ_LIMIT, **EVERY)
    _assert_same(got, cases.expect(key, ax.NX, ax.NY, 4, 8), CHECKED, f"{key} row share", rows)
    whole = scene(key).render_aov_through(_frame(cases, key, 4), 8, tx.FUZZ_LIMIT, ids=True)
    _assert_same(got, whole, ("prim", "inst"), f"{key} row share", rows)


@pytest.mark.parametrize("key", ax.PARITY)
def test_no_bounce_is_rt_render_aov(world, key):
    """max_bounces = 0: every output of rt_aov_desc is rt_render_aov's, nothing is followed -- on every parity scene."""
    cases, scene = world
    f = _frame(cases, key, 3)
    plain = scene(key).render_aov(f, ids=True)
    got = scene(key).render_aov_through(f, 0, 1.0, **EVERY)
    _assert_same(got, plain, tuple(plain), f"{key} max_bounces=0")
    assert not got["through"].any() and not got["bounces"].any()


def test_fuzz_limit_below_every_fuzz_is_rt_render_aov(world):
    """A glass-free scene whose metals are all fuzzier than the limit: nothing is followed at max_bounces = 8 either."""
    cases, scene = world
    f = _frame(cases, tx.NO_GLASS, 4)
    plain = scene(tx.NO_GLASS).render_aov(f, ids=True)
    got = scene(tx.NO_GLASS).render_aov_through(f, 8, tx.NO_GLASS_FUZZ_LIMIT, **EVERY)
    _assert_same(got, plain, tuple(plain), "no glass, low fuzz limit")
    assert not got["through"].any() and not got["bounces"].any()
    _assert_same(got, cases.expect(tx.NO_GLASS, ax.NX, ax.NY, 4, 8, tx.NO_GLASS_FUZZ_LIMIT), CHECKED, "no glass, low fuzz limit")
    # ... and with the limit raised its metals are followed: the same scene against the expectation
    far = scene(tx.NO_GLASS).render_aov_through(f, 8, 0.75, **EVERY)
    e = cases.expect(tx.NO_GLASS, ax.NX, ax.NY, 4, 8, 0.75)
    assert e["chain"]["metal_followed"].any() and e["chain"]["metal_unfollowed"].any()
    _assert_same(far, e, CHECKED, "no glass, fuzz limit 0.75")


@pytest.mark.parametrize("key", [tx.SPHERES, tx.GENERAL])
def test_each_output_alone(world, key):
    """Each output alone -- the kernel then skips what the others would need -- equals the same output among all of them."""
    cases, scene = world
    f = _frame(cases, key, 4)
    every = scene(key).render_aov_through(f, 8, tx.FUZZ_LIMIT, **EVERY)
    _assert_same(every, cases.expect(key, ax.NX, ax.NY, 4, 8), CHECKED, f"{key} all")
    for k in every:
        one = scene(key).render_aov_through(f, 8, tx.FUZZ_LIMIT, out={k: np.empty_like(every[k])})
        assert set(one) == {k} and np.array_equal(_bits(one[k]), _bits(every[k])), k


@pytest.mark.parametrize("key", [tx.SPHERES, tx.GENERAL])
def test_lds_modes_agree(gpu, world, key):
    """aov_through_lds -1, 0, 1 and 2."""
    cases, scene = world
    want = cases.expect(key, ax.NX, ax.NY, 4, 8)
    ref = None
    try:
        for lds in (-1, 0, 1, 2):
            gpu.set_option("aov_through_lds", lds)
            got = scene(key).render_aov_through(_frame(cases, key, 4), 8, tx.FUZZ_LIMIT, **EVERY)
            _assert_same(got, want, CHECKED, f"{key} aov_through_lds={lds}")
            ref = ref or got
            _assert_same(got, ref, ("prim", "inst"), f"{key} aov_through_lds={lds}")
    finally:
        gpu.reset_options()


def test_torch_tensors_on_a_side_stream(world):
    """out = torch device tensors: written in place, enqueued on the given stream, not waited for with blocking=False."""
    import torch
    cases, scene = world
    ds = scene(tx.GENERAL)
    want = cases.expect(tx.GENERAL, ax.NX, ax.NY, 4, 8)
    f = _frame(cases, tx.GENERAL, 4)
    dev = torch.device("cuda", ds.device)
    out = {k: torch.full((ax.NY, ax.NX, 3) if k in ("albedo", "normal") else (ax.NY, ax.NX), -7,
                         dtype=torch.float32 if k in FLOATS else torch.int32, device=dev) for k in CHECKED}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ret = ds.render_aov_through(f, 8, tx.FUZZ_LIMIT, out=out, stream=s, blocking=False)
    s.synchronize()
    assert ret is out
    _assert_same({k: v.cpu().numpy() for k, v in out.items()}, want, CHECKED, "torch, side stream")
    again = {"through": torch.zeros((ax.NY, ax.NX), dtype=torch.float32, device=dev)}
    torch.cuda.synchronize()
    ds.render_aov_through(f, 8, tx.FUZZ_LIMIT, out=again, stream=s.cuda_stream)          # an integer stream handle, blocking
    assert np.array_equal(_bits(again["through"].cpu().numpy()), _bits(want["through"]))
    with pytest.raises(ValueError):
        ds.render_aov_through(f, out={"through": torch.zeros((ax.NY, ax.NX), dtype=torch.float32)})      # a CPU tensor
    with pytest.raises(ValueError):
        ds.render_aov_through(f, out={"through": again["through"], "alpha": np.zeros((ax.NY, ax.NX), np.float32)})   # mixed


def test_rt_render_is_unchanged_by_the_pass(world):
    """rt_render of the same scene before and after a feature pass: the same frame and ray count."""
    cases, scene = world
    ds = scene(tx.SPHERES)
    frame = cases.case(tx.SPHERES).scene.frame(nx=ax.NX, ny=ax.NY, ns=8)
    before, st0 = ds.render(frame)
    ds.render_aov_through(_frame(cases, tx.SPHERES, 4), 8, tx.FUZZ_LIMIT, **EVERY)
    after, st1 = ds.render(frame)
    assert st0.rays == st1.rays and np.array_equal(_bits(before), _bits(after))


def test_render_denoised_takes_its_guides_from_the_pass(world):
    """render_denoised(through=True): the guides are render_aov_through's and the result is denoise() of them; off by default."""
    cases, scene = world
    ds = scene(tx.SPHERES)
    f = cases.case(tx.SPHERES).scene.frame(nx=ax.NX, ny=ax.NY, ns=4)
    r = ds.render_denoised(f, through=True, max_bounces=2, fuzz_limit=tx.FUZZ_LIMIT)
    f.gamma = 1.0
    guides = ds.render_aov_through(f, 2, tx.FUZZ_LIMIT, alpha=False)
    _assert_same(r, guides, ("albedo", "normal", "depth"), "render_denoised(through=True)")
    import accelerated_ray_tracer_amd as art
    assert np.array_equal(_bits(r["color"]), _bits(art.denoise(r["noisy"], guides["albedo"], guides["normal"], guides["depth"])))
    plain = ds.render_denoised(f)
    _assert_same(plain, ds.render_aov(f, alpha=False), ("albedo", "normal", "depth"), "render_denoised()")
    assert (_bits(plain["normal"]) != _bits(r["normal"])).any()


def test_cli_writes_the_same_buffers(gpu, tmp_path):
    """rayTracer --aov-through PREFIX: the four images are the binding's buffers, written as the image is."""
    nx, ny, ns = 40, 24, 3
    exe = os.path.join(gpu.LIB_DIR, "rayTracer")
    prefix = str(tmp_path / "cli")
    r = subprocess.run([exe, "--scene", "bouncing", "--nx", str(nx), "--ny", str(ny), "--ns", str(ns), "--p6", "--aov-through", prefix,
                        "--through-bounces", "3", "--through-fuzz", "0.5"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    hs = gpu.HostScene("bouncing", nx, ny)
    ds = gpu.DeviceScene(hs)
    try:
        got = ds.render_aov_through(hs.frame(ns=ns), 3, 0.5, alpha=False, through=True)
    finally:
        ds.close()
    assert got["through"].any()
    far = got["depth"].max()
    grey = lambda x: np.repeat(x[:, :, None], 3, axis=2)   # noqa: E731
    images = {"albedo": got["albedo"], "normal": np.float32(0.5) * got["normal"] + np.float32(0.5), "depth": grey(got["depth"] / far),
              "through": grey(got["through"])}
    for name, img in images.items():
        path = tmp_path / f"py.{name}.ppm"
        gpu.write_ppm(str(path), img, False, binary=True)
        assert path.read_bytes() == open(f"{prefix}.{name}.ppm", "rb").read(), name
    bad = subprocess.run([exe, "--nx", "16", "--ny", "8", "--ns", "2", "--through-bounces", "17", "--aov-through", prefix], capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"--through-bounces" in bad.stderr and bad.stdout == b""
    # --denoise-through: the filter is guided by the pass (a different frame than with the first-hit guides), and needs --denoise
    base = [exe, "--scene", "bouncing", "--nx", str(nx), "--ny", str(ny), "--ns", str(ns), "--p6", "--denoise"]
    plain = subprocess.run(base, capture_output=True, timeout=120)
    guided = subprocess.run(base + ["--denoise-through", "--through-fuzz", "0.5"], capture_output=True, timeout=120)
    assert plain.returncode == 0 and guided.returncode == 0, guided.stderr.decode()[-2000:]
    assert len(guided.stdout) == len(plain.stdout) and guided.stdout != plain.stdout
    alone = subprocess.run(base[:-1] + ["--denoise-through"], capture_output=True, timeout=60)
    assert alone.returncode == 2 and b"--denoise-through" in alone.stderr and alone.stdout == b""
