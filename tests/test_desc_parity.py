"""Parity on generated scene descriptions: the HIP kernels against the description oracle (OracleScene.from_desc).

rt_scene_create takes any well-formed rt_scene_desc; the named scenes are nineteen of them.  Here the descriptions come from
tests/scene_gen.py -- any hierarchy over the leaves, every mix of primitives, instances, media, materials and textures, any
camera -- and the checker is the oracle filled from the same description, itself anchored on the named oracle without a GPU
(tests/test_desc_oracle.py, which also holds the seed list and the conditions that keep these scenes from testing nothing).
Every comparison is bit-identical pixels and equal ray counts, as everywhere in this suite.
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_expect as ax
import scene_gen as sg
from test_desc_oracle import CASES, NS, NX, NY, ONE_SEED, SCHEDULE_EXTRA, SCHEDULE_FRAME
from test_gpu_parity import KERNELS, assert_frames_equal, render

pytestmark = pytest.mark.gpu
FLT_MAX = np.float32(np.finfo(np.float32).max)
ONE = [(r, ONE_SEED[r]) for r in sg.RECIPES]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def case(orc):
    """(generated scene, its description oracle, oracle frames by sample count) per (recipe, seed); computed once, left unchanged."""
    cache = {}

    class Case:
        def __init__(self, recipe, seed, nx, ny):
            self.g = sg.generate(recipe, seed, nx, ny)
            self.o = orc.OracleScene.from_host(self.g)
            self._ref = {}

        def ref(self, ns):
            if ns not in self._ref:
                self._ref[ns] = self.o.render(ns)
            return self._ref[ns]

    def get(recipe, seed, nx=NX, ny=NY):
        key = (recipe, seed, nx, ny)
        if key not in cache:
            cache[key] = Case(recipe, seed, nx, ny)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def rendered(gpu, case):
    """Default-option renders by (recipe, seed, kernel): (frame, rays, samples, kernel_variant)."""
    cache = {}

    def get(recipe, seed, kernel):
        key = (recipe, seed, kernel)
        if key not in cache:
            fb, st = render(gpu, case(recipe, seed).g, kernel, ns=NS)
            cache[key] = (fb, st.rays, st.samples, st.kernel_variant)
        return cache[key]
    return get


@pytest.mark.parametrize("recipe,seed", CASES)
def test_render_matches_description_oracle(case, rendered, recipe, seed):
    ref, cnt = case(recipe, seed).ref(NS)
    for kernel in KERNELS:
        fb, rays, samples, variant = rendered(recipe, seed, kernel)
        assert rays == cnt["rays"], (kernel, rays, cnt["rays"])
        assert samples == NX * NY * NS
        assert_frames_equal(fb, ref, f"{recipe}/{seed} kernel {kernel} variant {variant}")


def test_every_kernel_family_is_reached(rendered):
    """kernel_variant = kernel * 1000 + lds_mode * 100 + tex_level * 10 + spheres_only over the render cases: both families at
    texture levels 0, 1 and 2, the lockstep scan (LDS mode 4, the small `limits` scenes) and nodes and spheres in LDS (mode 2)."""
    seen = sorted({rendered(r, s, 3)[3] for r, s in CASES})
    fams = {(v % 10, v // 10 % 10) for v in seen}
    modes = {v // 100 % 10 for v in seen}
    assert {(so, lvl) for so in (0, 1) for lvl in (0, 1, 2)} <= fams, f"variants reached: {seen}"
    assert {2, 4} <= modes, f"variants reached: {seen}"
    assert all(v // 1000 == 3 for v in seen), seen
    assert {rendered(r, s, 0)[3] // 1000 for r, s in CASES} == {0}


def test_empty_description_renders_the_background(gpu, orc):
    """n_nodes = 0 is accepted (include/rt_abi.h): every ray misses, on both kernels the frame is the oracle's background."""
    g = sg.generate("spheres_plain", 1).emptied()
    ref, cnt = orc.OracleScene.from_host(g).render(NS)
    for kernel in KERNELS:
        fb, st = render(gpu, g, kernel, ns=NS)
        assert st.rays == cnt["rays"] == NX * NY * NS
        assert_frames_equal(fb, ref, f"empty scene, kernel {kernel}")


SCHEDULES = ({"split_samples": 4, "heavy_factor_x10": 15, "tier1_factor_x10": 25, "tier1_pixels": 64, "sparse_stride": 8},
             {"split_samples": 2, "heavy_factor_x10": 10, "tier1_factor_x10": 10, "tier1_pixels": 4096, "sparse_wg_percent": 100},
             {"split_samples": 4, "presplit_samples": 2, "heavy_factor_x10": 10, "tier1_factor_x10": 10, "tier1_pixels": 65536, "tier1_depth": 1, "sparse_work_percent": 100})
HANDOFF = {"handoff_pixels": 1 << 24, "handoff_poll_us": 1, "split_samples": 4}


@pytest.mark.parametrize("recipe,seed", ONE + SCHEDULE_EXTRA)
def test_schedule_and_handoff_match_description_oracle(gpu, case, recipe, seed):
    """The first, second and seventh option sets of test_split_frame_schedule_matches_oracle, and a hand-off of every pixel:
    scheduling only.  The hand-off runs exactly where the scene has tier data -- decided from the documented limits (at most
    4096 leaves, at most two media leaves: GenScene.has_tier_data), not from the run.  The frame is 64 x 64, the smallest the
    cost-aware schedule takes at all (rt_render ranks a frame of at least 64 tiles of 8 x 8 pixels; a 48 x 32 frame has 24 and
    would run as one plain launch whatever the options say)."""
    c = case(recipe, seed, *SCHEDULE_FRAME)
    ref, cnt = c.ref(8)
    for opts in SCHEDULES:
        fb, st = render(gpu, c.g, 3, opts, ns=8)
        assert st.rays == cnt["rays"], (opts, st.rays, cnt["rays"])
        assert_frames_equal(fb, ref, f"{recipe}/{seed} {opts}")
    L = gpu.rt_lib()
    L.rt_debug_handoff.argtypes = [C.c_void_p, C.c_void_p]
    gpu.reset_options()
    for k, v in HANDOFF.items():
        gpu.set_option(k, v)
    ds = gpu.DeviceScene(c.g)
    try:
        fb, st = ds.render(c.g.frame(ns=8))
        h = np.zeros(2, np.uint64)
        assert L.rt_debug_handoff(ds._p, h.ctypes.data) == 0
    finally:
        ds.close()
        gpu.reset_options()
    assert st.rays == cnt["rays"]
    assert_frames_equal(fb, ref, f"{recipe}/{seed} hand-off")
    print(recipe, seed, "handed off", int(h[0]), "tier data", c.g.has_tier_data)
    assert (int(h[0]) > 0) == c.g.has_tier_data, (int(h[0]), c.g.has_tier_data)


@pytest.mark.parametrize("recipe,seed", ONE)
def test_walk_array_is_invisible_on_any_tree(gpu, case, recipe, seed):
    """test_walk_array_is_invisible on a tree that is not the reference's median split: bvh_collapse 0..3 give the oracle's
    frame and ray count, and the walk array keeps every leaf."""
    c = case(recipe, seed)
    g = c.g
    ref, cnt = c.ref(NS)
    sizes = {}
    n_leaves = g.n_leaves
    for mode in (0, 1, 2, 3):
        gpu.reset_options()
        gpu.set_option("bvh_collapse", mode)
        ds = gpu.DeviceScene(g)
        try:
            info = ds.walk_info()
            gpu.reset_options()
            fb, st = ds.render(g.frame(ns=NS))
        finally:
            ds.close()
        assert st.rays == cnt["rays"], (mode, st.rays, cnt["rays"])
        assert_frames_equal(fb, ref, f"{recipe}/{seed} bvh_collapse={mode}")
        assert info["nodes_reference"] == g.desc.n_nodes
        sizes[mode] = info["nodes_walked"]
        assert n_leaves <= info["nodes_walked"] <= info["nodes_reference"]
        if mode and info["nodes_walked"] < info["nodes_reference"]:
            assert info["tests_after"] <= info["tests_before"]
    assert sizes[0] == g.desc.n_nodes
    print(recipe, seed, sizes)


def _query_rays(g, n=20000):
    """n rays, half camera rays (through random points of the image plane), half between random points of the root box, and
    n / 2 more among the objects; per-ray times inside the shutter."""
    rng = np.random.default_rng(len(g.name) + 7 * g.n_leaves)
    cam = g.desc.camera
    v = lambda a: np.array(list(a), np.float32)   # noqa: E731
    s, t = rng.random((2, n // 2, 1), dtype=np.float32)
    o1 = np.broadcast_to(v(cam.origin), (n // 2, 3))
    d1 = v(cam.lower_left_corner) + s * v(cam.horizontal) + t * v(cam.vertical) - v(cam.origin)
    root = g.nodes()[0]
    a = root["bmin"] + rng.random((n - n // 2, 3), dtype=np.float32) * (root["bmax"] - root["bmin"])
    b = root["bmin"] + rng.random((n - n // 2, 3), dtype=np.float32) * (root["bmax"] - root["bmin"])
    # The ground sphere (radius 200) makes the root box some 400 units wide, so the rays above mostly meet the ground alone:
    # half as many again run between random points of the box around every other leaf, where the objects stand.
    nodes = g.nodes()
    small = nodes[(nodes["prim"] >= 0) & ((nodes["bmax"] - nodes["bmin"]).max(1) < 100)]
    lo, hi = small["bmin"].min(0), small["bmax"].max(0)
    a2 = lo + rng.random((n // 2, 3), dtype=np.float32) * (hi - lo)
    b2 = lo + rng.random((n // 2, 3), dtype=np.float32) * (hi - lo)
    o = np.ascontiguousarray(np.concatenate([o1, a, a2]), np.float32)
    d = np.ascontiguousarray(np.concatenate([d1, b - a, b2 - a2]), np.float32)
    tm = (cam.time0 + rng.random(len(o)) * (cam.time1 - cam.time0)).astype(np.float32)
    assert np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).any(1).all()
    return o, d, tm


@pytest.mark.parametrize("recipe,seed", ONE)
def test_trace_matches_description_oracle(gpu, case, recipe, seed):
    """rt_trace_rays, closest hit with records and any-hit, default window, trace_lds -1 and 0: t, point, normal and uv bit for
    bit, the material as the description's index."""
    c = case(recipe, seed)
    o, d, tm = _query_rays(c.g)
    t, p, n, uv, mat = c.o.trace(o, d, tm)
    hit = t < FLT_MAX
    assert 0.2 < hit.mean(), float(hit.mean())          # (the ground fills the root box: most rays end somewhere)
    among = mat[20000:]
    assert len(among) == 10000 and len(np.unique(among[among >= 0])) >= min(3, c.g.desc.n_materials), np.unique(among)
    gpu.reset_options()
    ds = gpu.DeviceScene(c.g)
    try:
        for lds in (-1, 0):
            gpu.set_option("trace_lds", lds)
            r = ds.trace(o, d, tm, record=True)
            bad = np.flatnonzero(_bits(r.t) != _bits(t))
            assert len(bad) == 0, f"{recipe}/{seed} trace_lds {lds}: {len(bad)} rays differ in t, first {bad[:5]}: {r.t[bad[:5]]} vs {t[bad[:5]]}"
            assert np.array_equal(r.prim >= 0, hit)
            assert np.array_equal(_bits(r.point), _bits(p)) and np.array_equal(_bits(r.normal), _bits(n))
            assert np.array_equal(_bits(r.uv), _bits(uv))
            assert np.array_equal(r.mat, mat)
            assert np.array_equal(ds.trace(o, d, tm, any_hit=True), hit)
    finally:
        ds.close()
        gpu.reset_options()


FLOOR = 0.01


@pytest.mark.parametrize("recipe", ["general_tex", "media_many"])
def test_adaptive_matches_description_oracle(gpu, case, recipe):
    """rt_render_adaptive(min_spp 2, max_spp 16): every pixel, its count and the ray total as tests/adaptive_expect.py predicts
    them from the description oracle's renders."""
    c = case(recipe, ONE_SEED[recipe])
    ex = ax.Expectation(c.o)
    t = ex.threshold_with_spread(2, 16, FLOOR)
    assert t is not None, "no candidate threshold gives three distinct counts"
    gpu.reset_options()
    ds = gpu.DeviceScene(c.g)
    try:
        fb, spp, st = ds.render_adaptive(c.g.frame(ns=1), 2, 16, t, FLOOR)
    finally:
        ds.close()
    efb, espp, erays, esamples = ex.predict(2, 16, t, FLOOR, c.g.gamma)
    assert len(np.unique(espp)) >= 3
    assert np.array_equal(spp, espp), int((spp != espp).sum())
    bad = _bits(fb) != _bits(efb)
    assert not bad.any(), (int(bad.any(axis=-1).sum()), float(np.nanmax(np.abs(fb - efb))))
    assert st.rays == int(erays.sum()) and st.samples == int(esamples.sum())


@pytest.mark.parametrize("recipe", ["spheres_tex", "general_plain"])
def test_progressive_windows_match_description_oracle(gpu, case, recipe):
    """rt_render_window over [0, 3) and [3, 8): after each window the oracle's frame at that many samples; the rays add up."""
    c = case(recipe, ONE_SEED[recipe])
    gpu.reset_options()
    ds = gpu.DeviceScene(c.g)
    try:
        prog = ds.progressive(c.g.frame(ns=8))
        rays = 0
        for begin, end in ((0, 3), (3, 8)):
            fb, st = prog.render(begin, end)
            rays += st.rays
            ref, cnt = c.ref(end)
            assert rays == cnt["rays"], (end, rays, cnt["rays"])
            assert_frames_equal(fb, ref, f"{recipe} window [{begin}, {end})")
        prog.close()
    finally:
        ds.close()


def test_non_binary_hierarchy_is_a_legal_description(gpu, orc):
    """A root over three leaves (what the description oracle refuses, tests/test_desc_oracle.py) is still a legal walk: the
    product accepts it and renders what it renders for the binary tree over the same three leaves, interior boxes being
    invisible (rt_abi.hip, "Collapse")."""
    g = sg.generate("limits", 2)
    n = g.nodes()
    leaves = n[n["prim"] >= 0][:3]
    flat = np.zeros(4, gpu.NODE_DTYPE)
    flat[0] = (leaves["bmin"].min(0), 4, leaves["bmax"].max(0), -1)
    flat[1:] = leaves
    flat["skip"][1:] = [2, 3, 4]
    binary = np.zeros(5, gpu.NODE_DTYPE)
    binary[0] = flat[0]
    binary[1] = (leaves["bmin"][:2].min(0), 4, leaves["bmax"][:2].max(0), -1)
    binary[2:] = leaves
    binary["skip"][2:] = [3, 4, 5]
    binary["skip"][0] = 5
    frames = []
    for nodes in (flat, binary):
        a = dict(g._a, nodes=nodes)
        h = sg.GenScene("three", a, g.desc.camera, NX, NY, NS, g.gamma, g.background, g.use_gradient_bg, ())
        frames.append(render(gpu, h, 3, ns=NS) + (h,))
    assert frames[0][1].rays == frames[1][1].rays
    assert np.array_equal(_bits(frames[0][0]), _bits(frames[1][0]))
    ref, cnt = orc.OracleScene.from_host(frames[1][2]).render(NS)
    assert frames[1][1].rays == cnt["rays"]
    assert_frames_equal(frames[1][0], ref, "three leaves")


def _first(mask):
    return int(np.flatnonzero(mask)[0])


def _mutations(g):
    """(what validate() must say, field of the description, mutated array) -- one per invalid(...) branch of validate()."""
    t, ins, med, bx, n, m = g.textures(), g.instances(), g.media(), g.boxes(), g.nodes(), g.materials()
    checker, uvoff, image, noodle = (np.flatnonzero(t["kind"] == k) for k in (sg.T_CHECKER, sg.T_UVOFF, sg.T_IMAGE, sg.T_NOODLE))
    out = []

    def tex(what, index, **fields):
        x = t.copy()
        for k, v in fields.items():
            x[k][index] = v
        out.append((what, "textures", x))

    tex("checker children must be plain textures", checker[0], a=checker[1])
    tex("checker children must be plain textures", checker[0], b=uvoff[0])
    tex("image texture outside the image pool", image[0], a=g.desc.image_bytes - 1)
    tex("image texture with non-positive size", image[0], b=0)
    tex("image texture with non-positive size", image[1], c=-3)
    tex("noodle texture octaves out of range", noodle[0], a=17)
    tex("uv_offset may wrap", uvoff[0], a=checker[0])
    tex("unknown texture kind", 0, kind=7)
    x = ins.copy(); x["child"][0] = sg.ref(sg.INSTANCE, 1)
    out.append(("instance child must be a sphere, quad or box", "instances", x))
    x = med.copy(); x["boundary"][0] = sg.ref(sg.MEDIUM, 0)
    out.append(("medium boundary must be a sphere, quad, box or instance", "media", x))
    x = bx.copy(); x["first_quad"][-1] = g.desc.n_quads - 5
    out.append(("box faces out of range", "boxes", x))
    x = n.copy(); x["skip"][5] = 2
    out.append(("node skip link does not move forward", "nodes", x))
    x = n.copy(); x["skip"][0] = len(n) + 1
    out.append(("node skip link does not move forward", "nodes", x))
    x = m.copy(); x["kind"][3] = 5
    out.append(("unknown material kind", "materials", x))
    for field in ("spheres", "images"):
        out.append(("null array with non-zero count", field, None))
    return out


def test_validate_refuses_every_malformed_description(gpu, case):
    """One mutation of a generated general_tex description per invalid(...) branch of validate(): RT_ERR_INVALID, and
    rt_last_error_detail() names the failed check.  The unmutated description still creates and renders afterwards."""
    c = case("general_tex", ONE_SEED["general_tex"])
    g = c.g
    assert g.desc.n_media and g.desc.n_instances >= 2 and g.desc.n_boxes
    L = gpu.rt_lib()
    muts = _mutations(g)
    assert len({w for w, _, _ in muts}) == 12
    for what, field, arr in muts:
        d = gpu.RtSceneDesc.from_buffer_copy(g.desc)
        setattr(d, field, None if arr is None else arr.ctypes.data)
        p = C.c_void_p()
        st = L.rt_scene_create(C.byref(d), C.byref(p))
        detail = L.rt_last_error_detail().decode()
        if st == 0:
            L.rt_scene_destroy(p)
        assert st == 1, (what, field, st)                  # RT_ERR_INVALID
        assert what in detail, (what, detail)
    ref, cnt = c.ref(NS)
    fb, st = render(gpu, g, 3, ns=NS)
    assert st.rays == cnt["rays"]
    assert_frames_equal(fb, ref, "the unmutated description")
