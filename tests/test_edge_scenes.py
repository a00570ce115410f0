"""The edge scenes (tests/edge_scenes.py) on the kernels: frames in which equal t and exact boundaries decide every pixel.

Each scene sends every sample of every pixel along one exact primary ray, and tests/test_edge_scenes_host.py has shown from the
oracle alone that the scene's ties are bit-exact and that a planted error in the rule under test changes the frame.  Here every
frame must be the oracle's bit for bit with the oracle's ray count -- no tolerance anywhere:

  * kernel 0, the main kernel in every LDS mode the scene fits (the forced scan included) and created under bvh_collapse 0 .. 3
    (the deferred leaf tests and the regrouped or collapsed walk array must keep the reference's leaf order);
  * ranked 64 x 64 frames at 8 spp with every dear pixel on tier 1 and with every pixel handed off to the tail launch: the tier
    kernel's trace_wave decides ties by an order-independent reduction (rt_kernel_tier.h), which these frames
    hold to the sequence it replaces.  Every scene whose ray has three non-zero components takes them, and each asserts that
    pixels did reach the tier kernel, as tests/test_kernel_matrix.py does;
    the last test asserts that both trace_wave families and both LDS_SCENE instantiations were reached in this module;
  * the other consumers of the same device functions: rt_trace_rays on the primary ray (t, point, normal, uv, and the winner's
    material, which the description oracle reports by the description's own index), rt_radiance_rays, rt_render_aov at 1 spp.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import aov_expect as ax
import edge_scenes as es
import test_kernel_matrix_host as km
from test_gpu_parity import assert_frames_equal, render
from test_path_end import RANKED

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2, 3, 4)
SCAN_DEFAULT = 24                # rt_options::scan_nodes as shipped
OPTION_SETS = (("shipped", {}), ("one step a trip, leaf tests for all lanes at once", {"steps_per_trip": 1, "leaf_threshold": 64}))
# as tests/test_kernel_matrix.py: every pixel dearer than the mean on a tier wave beside the main kernel; every pixel on a tail wave
TIER_SETS = (("tier 1", dict(RANKED, tier_auto=0, tier1_pixels=65536, tier1_factor_x10=10)),
             ("handed off", dict(RANKED, handoff_pixels=1 << 24, handoff_poll_us=1)))
FLT_MAX = np.float32(np.finfo(np.float32).max)
SEEN_TIER = set()                # (spheres only, LDS_SCENE) where pixels did reach the tier kernel
# the padded scenes and the family each must select (sized as test_kernel_matrix_host.BIG's scenes of that family)
PADDED = {"padded/sphere-quad-sphere": "G,1", "padded/spheres-triple": "SO,1"}
# Scenes whose ranked frames are checked against the oracle and reach the tier kernel in neither: every path has the same length
# (rays per sample below), so no pixel is dearer than the mean and no wave runs dry before the others.  A light ends every path
# at the first hit; the glass quad reflects every path but one into the sky.  Their rules reach trace_wave through other scenes:
# texture lookups do not pass through it, and glass on a tier wave is in the generated scenes of tests/test_desc_parity.py.
NEVER_ON_TIER = {"texture/image-light": 1, "texture/checker-light": 1, "seeded/glass-uniform-1": 2}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _base(gpu, orc, e, nx, ny, ns):
    """The scene at a frame size: the oracle's frame and ray count, and kernel 0's frame, which must be the oracle's."""
    hs = e.build(nx, ny, ns)
    ref, cnt = orc.OracleScene.from_host(hs).render(ns, seed_base=e.seed_base)
    fb0, st0 = render(gpu, hs, 0, ns=ns, seed_base=e.seed_base)
    assert st0.rays == cnt["rays"], (e.name, st0.rays, cnt["rays"])
    assert st0.kernel_variant // 1000 == 0, st0.kernel_variant
    assert_frames_equal(fb0, ref, f"{e.name} kernel 0")
    return SimpleNamespace(key=e.name, hs=hs, f=km.facts(gpu, hs), ref=ref, rays=cnt["rays"], fb0=fb0, ns=ns, seed=e.seed_base)


def _options(gpu, opts):
    gpu.reset_options()
    for k, v in opts.items():
        gpu.set_option(k, v)
    if any(k.startswith(("tier1_", "heavy_")) for k in opts):
        gpu.set_option("tier_auto", 0)


def _create(gpu, hs, **creation_opts):
    """A DeviceScene created under the shipped options plus `creation_opts`; the options are the shipped ones again afterwards."""
    _options(gpu, creation_opts)
    try:
        return gpu.DeviceScene(hs)
    finally:
        gpu.reset_options()


def _frame(gpu, ds, b, opts):
    """One frame of a resident scene with the staged kernel under the shipped options plus `opts`."""
    _options(gpu, dict(opts, kernel=3))
    try:
        return ds.render(b.hs.frame(ns=b.ns, seed_base=b.seed))
    finally:
        gpu.reset_options()


def _walked(ds, b):
    n = ds.walk_info()["nodes_walked"]
    assert b.f["n_leaves"] <= n <= b.f["n_nodes"], (b.key, n, b.f)
    return n


def _check(b, fb, st, mode, what):
    """The frame is kernel 0's and the oracle's, the rays are the oracle's, and the instantiation is the one the rule predicts."""
    assert st.kernel_variant == km.expected_variant(mode, b.f), (what, st.kernel_variant, km.expected_variant(mode, b.f))
    assert st.rays == b.rays, (what, st.rays, b.rays)
    assert st.samples == b.ref.shape[0] * b.ref.shape[1] * b.ns, what
    assert np.array_equal(fb.view(np.uint32), b.fb0.view(np.uint32)), what
    assert_frames_equal(fb, b.ref, what)


@pytest.mark.parametrize("name", [e.name for e in es.EDGES])
def test_frame_in_every_mode(gpu, orc, name):
    """16 x 16 at 8 spp: kernel 0; the library's mode; lds_mode 0 .. 4; creations under bvh_collapse 0 .. 3, walked and scanned."""
    e = es.BY_NAME[name]
    b = _base(gpu, orc, e, es.NX, es.NY, es.NS)
    ds = _create(gpu, b.hs)
    try:
        n = _walked(ds, b)
        fb, st = _frame(gpu, ds, b, {})
        _check(b, fb, st, km.expected_mode(-1, SCAN_DEFAULT, n, b.f), f"{name}: the library's mode")
        for mode in MODES:
            assert km.mode_fits(mode, n, b.f), (name, mode)
            for tag, opts in OPTION_SETS:
                fb, st = _frame(gpu, ds, b, dict(opts, lds_mode=mode))
                _check(b, fb, st, mode, f"{name} lds_mode {mode}: {tag}")
    finally:
        ds.close()
    for collapse in (0, 1, 2, 3):
        ds = _create(gpu, b.hs, bvh_collapse=collapse)
        try:
            _walked(ds, b)
            for mode in (2, 4):
                fb, st = _frame(gpu, ds, b, {"lds_mode": mode})
                _check(b, fb, st, mode, f"{name} created under bvh_collapse {collapse}, lds_mode {mode}")
        finally:
            ds.close()


def _ranked(gpu, b, tag, opts):
    """A ranked frame under `opts` (created and rendered under them, as rt_render's callers do): the frame is the oracle's, the
    tier kernel's room is the restated plan's (tests/test_kernel_matrix_host.py), and pixels did reach the tier kernel -- as
    tier 1 of the last part's ranking, or from the tail queue.  Returns LDS_SCENE."""
    L = gpu.rt_lib()
    L.rt_debug_handoff.argtypes = [C.c_void_p, C.c_void_p]
    _options(gpu, dict(opts, kernel=3))
    ds = gpu.DeviceScene(b.hs)
    try:
        n = _walked(ds, b)
        room = ds.tier_room()
        fb, st = ds.render(b.hs.frame(ns=b.ns, seed_base=b.seed))
        h = np.zeros(2, np.uint64)
        assert L.rt_debug_handoff(ds._p, h.ctypes.data) == 0
        info = np.zeros(13, np.uint32)                             # the frame's last ranking: [2] = pixels it gave to tier 1
        tier1 = int(info[2]) if L.rt_debug_rank_info(ds._p, info.ctypes.data) == 0 else 0
    finally:
        ds.close()
        gpu.reset_options()
    handed = int(h[0])
    what = f"{b.key}: {tag}"
    mode = opts["lds_mode"]
    print(what, "variant", st.kernel_variant, "rays per sample", round(b.rays / (b.ref.shape[0] * b.ref.shape[1] * b.ns), 2), "tier 1 pixels", tier1,
          "handed off", handed, "room", room)
    _check(b, fb, st, mode, what)
    fits, scene, lds, per_cu = km.tier_room(b.f, km.main_lds_bytes(mode, n, b.f))
    assert (room["fits"], room["lds_scene"], room["lds"]) == (fits, scene, lds) and fits, (what, room, (fits, scene, lds))
    # Handed off, every pixel leaves for the tail launch after its first sample: the tier kernel is reached in every scene.  Tier 1
    # is the ranking's choice among measured costs: in a frame whose pixels cost alike (every path ends at its first hit, or
    # every path runs to the bounce limit) it finds no pixel dearer than the mean, so it must be non-empty only where the
    # scene's far fillers and ground make the pixels differ -- the scenes of at least 65 leaves, and the padded ones.
    # A pixel is handed off when its wave runs dry while others still render: where every path of the frame has the same length
    # no wave ever does, and no schedule brings such a frame to the tier kernel.  NEVER_ON_TIER names those scenes.
    samples = b.ref.shape[0] * b.ref.shape[1] * b.ns
    if b.key in NEVER_ON_TIER:
        assert abs(b.rays - NEVER_ON_TIER[b.key] * samples) <= 50, (what, b.rays, samples)   # (all paths but the seeded one)
    if tag == "handed off":
        assert handed > 0 or b.key in NEVER_ON_TIER, what
    elif b.f["n_leaves"] >= 65:
        assert tier1 > 0, what
    if handed > 0 or tier1 > 0:
        SEEN_TIER.add((b.f["spheres_only"], scene))
    return scene


# every scene whose ray has three non-zero components (a zero component sends the tier wave to the reference walk)
RANKED_SCENES = [e.name for e in es.EDGES if (e.d != 0).all()]


@pytest.mark.parametrize("name", RANKED_SCENES)
def test_ranked_frame_on_the_tier_kernel(gpu, orc, name):
    """64 x 64 at 8 spp, the main kernel walking (lds_mode 2: the library would scan the small scenes, and a scanned frame has no
    tier 1): every pixel dearer than the mean on a tier wave; every pixel handed off.  Both frames must be the oracle's; pixels
    must have reached the tier kernel in the second, and in the first too where the scene has 65 leaves or more (_ranked)."""
    e = es.BY_NAME[name]
    b = _base(gpu, orc, e, km.SNX, km.SNY, km.SNS)
    for tag, opts in TIER_SETS:
        assert _ranked(gpu, b, tag, dict(opts, split_samples=4, lds_mode=2)) is True


@pytest.mark.parametrize("name", list(PADDED))
def test_ranked_frame_with_the_scene_in_global_memory(gpu, orc, name):
    """The tie among thousands of far spheres: the tier kernel's leaf arrays fit its room, the records do not (LDS_SCENE = false).
    Frames and options as test_kernel_matrix's test_tier_kernel_with_the_scene_in_global_memory."""
    e = es.BY_NAME[name]
    for (tag, opts), ns in zip(TIER_SETS, (2, 4)):
        b = _base(gpu, orc, e, km.SNX, km.SNY, ns)
        assert b.f["family"] == PADDED[name], b.f
        assert _ranked(gpu, b, tag, dict(opts, split_samples=ns // 2, **km.BIG_OPTS)) is False


@pytest.mark.parametrize("name", [e.name for e in es.EDGES + es.PADDED])
def test_queries_on_the_primary_ray(gpu, orc, name):
    """rt_trace_rays, rt_radiance_rays and rt_render_aov meet the same ray through the same device functions."""
    e = es.BY_NAME[name]
    hs = e.scene
    whole = orc.OracleScene.from_host(hs)
    o, d = np.tile(e.o, (5, 1)), np.tile(e.d, (5, 1))
    t, p, n, uv, mat = whole.trace(o, d)
    if e.winner_mat is not None:
        assert (mat == e.winner_mat).all()
    ds = gpu.DeviceScene(hs)
    try:
        r = ds.trace(o, d, record=True)
        hit = t < FLT_MAX
        assert np.array_equal(_bits(r.t), _bits(t)), (name, r.t, t)
        for got, want, what in ((r.point, p, "point"), (r.normal, n, "normal"), (r.uv, uv, "uv")):
            assert np.array_equal(_bits(got), _bits(np.where(hit[:, None], want, np.float32(0)))), (name, what, got[0], want[0])
        assert np.array_equal(r.mat, np.where(hit, mat, -1)), (name, r.mat, mat)
        assert np.array_equal(ds.trace(o, d, any_hit=True), hit), name
        # radiance: per query the oracle's 1 x 1 frame of this very camera at the query's seed and gamma 1
        seeds = np.array([1984, 1985, 7, 77_000_000_019, 2 ** 63 + 5], np.uint64)
        one = orc.OracleScene.from_desc(hs.desc, 1, 1, 1.0, hs.background, hs.use_gradient_bg)
        rad = ds.radiance(o, d, ns=es.NS, seeds=seeds, count_rays=True)
        for k, s in enumerate(seeds):
            fb, cnt = one.render(es.NS, gamma=1.0, seed_base=int(s), threads=1)
            assert np.array_equal(_bits(rad.rgb[k]), _bits(fb[0, 0])), (name, k, rad.rgb[k], fb[0, 0])
            assert int(rad.rays[k]) == cnt["rays"], (name, k)
        # feature buffers at 1 spp: albedo, normal, depth, coverage and the winner's material
        want = ax.expected(orc, hs, es.NX, es.NY, 1, gpu, whole)
        got = ds.render_aov(hs.frame(nx=es.NX, ny=es.NY, ns=1, seed_base=ax.SEED), ids=True)
        for k in ("albedo", "normal", "depth", "alpha"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (name, k)
        assert np.array_equal(got["mat"], want["mat"]), (name, got["mat"][0, 0], want["mat"][0, 0])
        if e.winner_mat is not None:
            assert (got["mat"] == e.winner_mat).all(), (name, got["mat"][0, 0], e.winner_mat)
    finally:
        ds.close()


def test_both_families_and_both_scene_placements_ran(gpu):
    """trace_wave's spheres-only and general families, each with the scene records in LDS and in global memory."""
    print("tier kernel:", sorted(SEEN_TIER))
    assert SEEN_TIER == {(so, scene) for so in (True, False) for scene in (True, False)}, \
        f"{sorted(SEEN_TIER)} (filled by the ranked tests of this module: run it whole, not under -k)"
