"""Every instantiation of the main kernel and of the tier kernel, on the scenes that carry each family's difficult content.

The main kernel exists 25 times -- five families (spheres only at texture levels 0, 1 and 2; general at levels 1 and 2) times five
LDS modes (rt_kernel_staged.h: 0 nothing in LDS, 1 the walk array, 2 and the spheres, 3 and materials and textures, 4 the lockstep
scan, which replaces stages A and B) --, the tier kernel ten times: the same families with the scene records in its LDS image or
read from global memory (LDS_SCENE).  One text each, but every mode stages the scene with loops of its own, and the rest of the
suite forces modes on built-in scenes only and renders the generated ones in the library's choice of mode only.

What can go wrong: a wrong count in a staging loop, a stale or altered record in an LDS copy, a wrong skip in the scan (whose
interior-node branch only runs where the array still has interior nodes: a creation under bvh_collapse 0 or scan_nodes 0, or a
forced lds_mode 4), a mode leaving state behind on a resident scene, a create/render mismatch of scan_nodes.  So: one scene per
family (tests/test_kernel_matrix_host.py pins which), rendered by the oracle and by kernel 0 once, then in every mode under option
sets that change when the stages run; every frame must be kernel 0's and the oracle's bit for bit with the oracle's ray count, and
`kernel_variant` must name the instantiation the planning rule predicts -- computed from the description (the restated rules of
the host module), never read back from the run.  The last test asserts that all 25 + 10 instantiations did run in this module,
and a forced scan over interior nodes in each family.

profiles/kernel_matrix_tests_mutations.md: what these cases catch that the others let through, and each case's wall time.
"""
import ctypes as C
import time
from types import SimpleNamespace

import numpy as np
import pytest

import test_kernel_matrix_host as km
from test_gpu_parity import assert_frames_equal, render
from test_path_end import OPTION_SETS as PATH_END_SETS, RANKED, _render

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2, 3, 4)
OPTION_SETS = (("shipped", {}),
               ("one step a trip, leaf tests for all lanes at once", {"steps_per_trip": 1, "leaf_threshold": 64}),
               ("leaf tests for one lane", {"leaf_threshold": 1}))
# test_path_end's: every pixel leaves for the tail launch after its first sample; parts, tiers, sparse and semi waves
SCHEDULED_SETS = tuple((tag, opts) for tag, opts in PATH_END_SETS if tag in ("handed off", "split"))
assert len(SCHEDULED_SETS) == 2
# the tier kernel: every pixel dearer than the mean on a tier wave beside the main kernel; every pixel on a tail wave
TIER_SETS = (("tier 1", dict(RANKED, tier_auto=0, tier1_pixels=65536, tier1_factor_x10=10)),
             ("handed off", dict(RANKED, handoff_pixels=1 << 24, handoff_poll_us=1)))
SCAN_DEFAULT = 24                # rt_options::scan_nodes as shipped

SEEN_MAIN = set()                # (family, mode, the array had interior nodes)
SEEN_TIER = set()                # (family, LDS_SCENE), where pixels did reach the tier kernel
TIMES = {}                       # wall seconds per case


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    TIMES[request.node.name] = time.perf_counter() - t0


@pytest.fixture(scope="module")
def base(gpu, orc):
    """Per (scene, frame): the description's facts, the oracle's frame and ray count, and kernel 0's frame -- which must be the
    oracle's --, computed once and left unchanged."""
    cache = {}

    def get(key, nx=km.NX, ny=km.NY, ns=km.NS):
        k = (key, nx, ny, ns)
        if k not in cache:
            hs = km.big_scene(key[4:], nx, ny) if key.startswith("big/") else km.load(gpu, key, nx, ny)
            ref, cnt = km.oracle_of(orc, gpu, key, hs, nx, ny).render(ns)
            fb0, st0 = render(gpu, hs, 0, ns=ns)
            assert st0.rays == cnt["rays"], (key, st0.rays, cnt["rays"])
            assert st0.kernel_variant // 1000 == 0, st0.kernel_variant
            assert_frames_equal(fb0, ref, f"{key} kernel 0")
            cache[k] = SimpleNamespace(key=key, hs=hs, f=km.facts(gpu, hs), ref=ref, rays=cnt["rays"], fb0=fb0, ns=ns)
        return cache[k]
    return get


def _create(gpu, hs, **creation_opts):
    """A DeviceScene created under the shipped options plus `creation_opts`; the options are the shipped ones again afterwards."""
    gpu.reset_options()
    for k, v in creation_opts.items():
        gpu.set_option(k, v)
    try:
        return gpu.DeviceScene(hs)
    finally:
        gpu.reset_options()


def _frame(gpu, ds, b, opts):
    """One frame of a resident scene with the staged kernel under the shipped options plus `opts`."""
    gpu.reset_options()
    gpu.set_option("kernel", 3)
    for k, v in opts.items():
        gpu.set_option(k, v)
    try:
        return ds.render(b.hs.frame(ns=b.ns))
    finally:
        gpu.reset_options()


def _check(b, fb, st, mode, what, n_walked):
    """The frame is kernel 0's and the oracle's, the rays are the oracle's, and the instantiation is the one the rule predicts."""
    assert st.kernel_variant == km.expected_variant(mode, b.f), (what, st.kernel_variant, km.expected_variant(mode, b.f))
    assert st.rays == b.rays, (what, st.rays, b.rays)
    assert st.samples == b.ref.shape[0] * b.ref.shape[1] * b.ns, what
    assert np.array_equal(fb.view(np.uint32), b.fb0.view(np.uint32)), what
    assert_frames_equal(fb, b.ref, what)
    SEEN_MAIN.add((b.f["family"], mode, n_walked > b.f["n_leaves"]))


def _walked(ds, b):
    n = ds.walk_info()["nodes_walked"]
    assert b.f["n_leaves"] <= n <= b.f["n_nodes"], (b.key, n, b.f)
    return n


@pytest.mark.parametrize("key", list(km.SCENES))
def test_every_mode(gpu, base, key):
    """lds_mode 0 .. 4 set after a default creation, under three option sets; and the library's own choice of mode."""
    b = base(key)
    ds = _create(gpu, b.hs)
    try:
        n = _walked(ds, b)
        fb, st = _frame(gpu, ds, b, {})
        _check(b, fb, st, km.expected_mode(-1, SCAN_DEFAULT, n, b.f), f"{key}: the library's mode", n)
        for mode in MODES:
            assert km.mode_fits(mode, n, b.f), (key, mode)         # (every scene here fits every mode)
            for tag, opts in OPTION_SETS:
                fb, st = _frame(gpu, ds, b, dict(opts, lds_mode=mode))
                _check(b, fb, st, mode, f"{key} lds_mode {mode}: {tag}", n)
    finally:
        ds.close()


@pytest.mark.parametrize("key", list(km.SCENES))
def test_every_mode_on_a_ranked_frame(gpu, base, key):
    """The same on 64 x 64 at 8 spp, the smallest frame the cost-aware schedule ranks, with every pixel handed off to the tail
    launch after its first sample, and with parts, tiers, sparse and semi waves.  Pixels never leave where the tier kernel's
    image has no room beside the main kernel's (the restated plan_tier_room), and in the five family scenes always where it has."""
    b = base(key, km.SNX, km.SNY, km.SNS)
    ds = _create(gpu, b.hs)
    n = _walked(ds, b)
    ds.close()
    for mode in MODES:
        fits = km.tier_room(b.f, km.main_lds_bytes(mode, n, b.f))[0]
        for tag, opts in SCHEDULED_SETS:
            fb, st, handed = _render(gpu, b.hs, dict(opts, lds_mode=mode), b.ns)
            what = f"{key} lds_mode {mode}: {tag}"
            print(what, "variant", st.kernel_variant, "rays", st.rays, "handed off", handed)
            _check(b, fb, st, mode, what, n)
            if tag == "handed off":
                assert handed == 0 or fits, (what, handed)
                # (asserted where pixels differ enough in cost for a wave to run dry while its neighbours still render: in
                # `degenerate`, as in test_path_end, or in a one-sphere scene every pixel may be over before a wave looks)
                if key in km.FAMILY_SCENE.values():
                    assert handed > 0, (what, handed)


@pytest.mark.parametrize("key", [k for k in km.SCENES if km.SCENES[k][3] >= 2])
def test_scan_over_an_array_with_interior_nodes(gpu, base, key):
    """lds_mode 4 forced on arrays the scan was not prepared for: the planner's array, kept whole by a creation under scan_nodes 0,
    and the reference tree itself (bvh_collapse 0).  The scan's interior branch -- a lane skips the subtree of a box it failed --
    runs only here; in the zero-direction scenes together with the reference form of the box test."""
    b = base(key)
    for creation in ({"scan_nodes": 0}, {"bvh_collapse": 0}):
        ds = _create(gpu, b.hs, **creation)
        try:
            n = _walked(ds, b)
            if "bvh_collapse" in creation:
                assert n == b.f["n_nodes"] > b.f["n_leaves"], (key, n)
            elif key in km.FAMILY_SCENE.values():
                assert n > b.f["n_leaves"], (key, creation, n)      # the planner keeps some interior node of a hundred-leaf tree
            for tag, opts in OPTION_SETS[:2]:
                fb, st = _frame(gpu, ds, b, dict(opts, lds_mode=4))
                _check(b, fb, st, 4, f"{key} created under {creation}, scanned: {tag}", n)
        finally:
            ds.close()


@pytest.mark.parametrize("key", km.SCAN_RENDER_SCENES)
def test_scan_nodes_at_render_time(gpu, base, key):
    """Created at the defaults, rendered under scan_nodes 0, n - 1, n and 64 (n = the array's nodes): scanned exactly when
    0 < n <= scan_nodes, otherwise in the mode the size rule gives."""
    b = base(key)
    ds = _create(gpu, b.hs)
    try:
        n = _walked(ds, b)
        values = sorted({s for s in (0, n - 1, n, 64) if 0 <= s <= 64})     # (the option's range)
        assert {0, 64} <= set(values)
        for s in values:
            fb, st = _frame(gpu, ds, b, {"scan_nodes": s})
            mode = km.expected_mode(-1, s, n, b.f)
            assert (mode == 4) == (0 < n <= s) and (mode == 4 or mode == 2), (key, s, n, mode)
            _check(b, fb, st, mode, f"{key}: {n} nodes rendered under scan_nodes {s}", n)
    finally:
        ds.close()


@pytest.mark.parametrize("key", km.SCAN_RENDER_SCENES)
def test_scan_nodes_at_creation(gpu, base, key):
    """Created under scan_nodes 64: an array of at most 64 nodes comes back as its leaves, a larger one untouched.  Rendered under
    other values and forced modes -- a leaves-only array walked, a whole array scanned -- the frames stay the oracle's: a
    create/render mismatch costs box tests and never pixels."""
    b = base(key)
    ds = _create(gpu, b.hs, scan_nodes=0)
    n0 = _walked(ds, b)
    ds.close()
    ds = _create(gpu, b.hs, scan_nodes=64)
    try:
        n = _walked(ds, b)
        assert n == (b.f["n_leaves"] if n0 <= 64 else n0), (key, n0, n, b.f["n_leaves"])
        for s in (0, 24, 64):
            for lds_mode in (-1, 0, 2, 4):
                fb, st = _frame(gpu, ds, b, {"scan_nodes": s, "lds_mode": lds_mode})
                _check(b, fb, st, km.expected_mode(lds_mode, s, n, b.f), f"{key}: created under scan_nodes 64 ({n} nodes), rendered under {s}, lds_mode {lds_mode}", n)
    finally:
        ds.close()


@pytest.mark.parametrize("key", list(km.SCENES))
def test_modes_in_sequence_on_one_resident_scene(gpu, base, key):
    """Modes 4, 2, 0, 3, 1, 4 on one DeviceScene: every frame is the first's.  A mode that left state behind would show."""
    b = base(key)
    ds = _create(gpu, b.hs)
    try:
        n = _walked(ds, b)
        first = None
        for step, mode in enumerate((4, 2, 0, 3, 1, 4)):
            fb, st = _frame(gpu, ds, b, {"lds_mode": mode})
            _check(b, fb, st, mode, f"{key} step {step}: lds_mode {mode}", n)
            first = fb if first is None else first
            assert np.array_equal(fb.view(np.uint32), first.view(np.uint32)), (key, step, mode)
    finally:
        ds.close()


def _render_room(gpu, hs, opts, ns):
    """test_path_end's _render, plus the tier kernel's room as the frame's plan had it (rt_debug_tier_room under the same options)."""
    L = gpu.rt_lib()
    L.rt_debug_handoff.argtypes = [C.c_void_p, C.c_void_p]
    gpu.reset_options()
    gpu.set_option("kernel", 3)
    for k, v in opts.items():
        gpu.set_option(k, v)
    if any(k.startswith(("tier1_", "heavy_")) for k in opts):
        gpu.set_option("tier_auto", 0)
    ds = gpu.DeviceScene(hs)
    try:
        n = ds.walk_info()["nodes_walked"]
        room = ds.tier_room()
        fb, st = ds.render(hs.frame(ns=ns))
        h = np.zeros(2, np.uint64)
        assert L.rt_debug_handoff(ds._p, h.ctypes.data) == 0
        assert ds.tier_room() == room                              # the diagnostic launches nothing and leaves the scene alone
        info = np.zeros(13, np.uint32)                             # the frame's last ranking: [2] = pixels it gave to tier 1
        tier1 = int(info[2]) if L.rt_debug_rank_info(ds._p, info.ctypes.data) == 0 else 0
    finally:
        ds.close()
        gpu.reset_options()
    return fb, st, int(h[0]), tier1, room, n


def _check_tier(gpu, b, sets, want_scene):
    for tag, opts in sets:
        fb, st, handed, tier1, room, n = _render_room(gpu, b.hs, opts, b.ns)
        what = f"{b.key}: {tag}"
        mode = km.expected_mode(opts.get("lds_mode", -1), SCAN_DEFAULT, n, b.f)
        print(what, "variant", st.kernel_variant, "tier 1 pixels", tier1, "handed off", handed, "room", room)
        _check(b, fb, st, mode, what, n)
        fits, scene, lds, per_cu = km.tier_room(b.f, km.main_lds_bytes(mode, n, b.f))
        assert (room["fits"], room["lds_scene"], room["lds"]) == (fits, scene, lds) == (True, want_scene, lds), (what, room, (fits, scene, lds))
        assert room["tail_grid"] > 0 and room["tail_grid"] % per_cu == 0, (what, room, per_cu)
        # pixels did reach this instantiation of the tier kernel: from the tail queue, or as tier 1 of the last part's ranking
        # (a scanned scene has no tier 1: plan_frame)
        if tag == "handed off":
            assert handed > 0, what
        elif mode != 4:
            assert tier1 > 0, what
        if handed > 0 or tier1 > 0:
            SEEN_TIER.add((b.f["family"], room["lds_scene"]))


@pytest.mark.parametrize("family", km.FAMILIES)
def test_tier_kernel_with_the_scene_in_lds(gpu, base, family):
    """LDS_SCENE = true: each family's scene with every dear pixel on a tier wave beside the main kernel, then with every pixel
    handed off to the tail launch."""
    b = base(km.FAMILY_SCENE[family], km.SNX, km.SNY, km.SNS)
    _check_tier(gpu, b, [(tag, dict(opts, split_samples=4)) for tag, opts in TIER_SETS], True)


@pytest.mark.parametrize("family", km.FAMILIES)
def test_tier_kernel_with_the_scene_in_global_memory(gpu, base, family):
    """LDS_SCENE = false: a few thousand small spheres (with a quad in the general families), whose leaf arrays fit the tier
    kernel's room and whose records do not -- the host module sizes them from rt_tier_lds_bytes.  64 x 64 at 2 spp, the main
    kernel with nothing in LDS; the array is walked, not scanned.  At 2 spp the two parts hold one sample each, so tier 1 of the
    second part is what reaches the tier kernel; a pixel can only be handed off with samples left to go, so the hand-off runs
    at 4 spp in parts of two."""
    for (tag, opts), ns in zip(TIER_SETS, (2, 4)):
        b = base("big/" + family, km.SNX, km.SNY, ns)
        assert b.f["family"] == family
        _check_tier(gpu, b, [(tag, dict(opts, split_samples=ns // 2, **km.BIG_OPTS))], False)


def test_every_instantiation_ran(gpu):
    """All 25 (family, mode) pairs of the main kernel, a scan over interior nodes in every family, all 10 of the tier kernel."""
    main = {(fam, mode) for fam, mode, _ in SEEN_MAIN}
    scans = {fam for fam, mode, interior in SEEN_MAIN if mode == 4 and interior}
    print("main kernel:", sorted(main))
    print("scans over interior nodes:", sorted(scans))
    print("tier kernel:", sorted(SEEN_TIER))
    for name, seconds in sorted(TIMES.items(), key=lambda x: -x[1]):
        print(f"{seconds:7.2f} s  {name}")
    assert main == {(fam, mode) for fam in km.FAMILIES for mode in MODES}, sorted({(f, m) for f in km.FAMILIES for m in MODES} - main)
    assert scans == set(km.FAMILIES), scans
    assert SEEN_TIER == {(fam, scene) for fam in km.FAMILIES for scene in (True, False)}, SEEN_TIER
