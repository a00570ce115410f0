"""The premises of tests/test_kernel_matrix.py, from the scene descriptions alone: no device.

That module renders one scene per kernel family in every LDS mode and reads off `kernel_variant` which instantiation ran.  What
it takes for granted is pinned here: which family each scene's description selects (rt_abi.hip, validate() and launch_render()),
its leaf and node counts, the media of the `general_*` seeds, the zero-direction cameras, and -- for the scenes built to push the
tier kernel into its `LDS_SCENE = false` instantiations -- that the leaf arrays fit the tier kernel's room and the scene records
beside them do not.  The planning rules are restated here in Python from rt_frame_plan.h and rt_device.h (the GPU module compares
the restatement with what the library reports: kernel_variant, rt_debug_tier_room); the scene table and the builders are shared
with the GPU module, which imports them from here.
"""
import ctypes as C

import numpy as np
import pytest

import scene_gen as sg

LDS_PER_CU = 160 * 1024          # bytes of LDS per CU of this part (gfx950)
NX, NY, NS = 48, 32, 4           # the matrix frame: 24 work tiles, one plain launch whatever the options say
SNX, SNY, SNS = 64, 64, 8        # 64 work tiles: the smallest frame the cost-aware schedule ranks
FAMILIES = ("SO,0", "SO,1", "SO,2,uv", "G,1", "G,2,uv")   # rt_launch_staged_family's five; the tier kernel's five

# scene: (family, spheres_only, tex_level, leaves, what it is there for).  generated scenes: 2 * leaves - 1 nodes
SCENES = {
    "spheres_plain/1": ("SO,0", 1, 0, 106, "moving spheres, metal, glass"),
    "spheres_checker/1": ("SO,1", 1, 1, 105, "checker textures"),
    "spheres_tex/1": ("SO,2,uv", 1, 2, 71, "all seven texture kinds"),
    "earth": ("SO,2,uv", 1, 2, 1, "image uv"),
    "perlin": ("SO,2,uv", 1, 2, 2, "noise"),
    "general_plain/1": ("G,1", 0, 1, 25, "quads, boxes, instances of every kind; two media"),
    "general_plain/3": ("G,1", 0, 1, 27, "the same, no medium"),
    "general_tex/4": ("G,2,uv", 0, 2, 30, "the same under textures; two media"),
    "general_tex/3": ("G,2,uv", 0, 2, 39, "the same under textures, no medium"),
    "media_many/0": ("G,1", 0, 0, 26, "camera inside a medium; no tier data"),
    "degenerate": ("SO,0", 1, 0, 5, "zero direction components: both trips in one wave"),
    "bouncing/parallel": ("SO,1", 1, 1, 488, "every camera ray has two zero direction components"),
    "quad_edge": ("G,1", 0, 0, 8, "rays with a zero y direction in the plane of a box's upper face: 0 * inf in the box test"),
    "limits/4": ("SO,0", 1, 0, 24, "47 reference nodes"),
    "limits/5": ("SO,0", 1, 0, 25, "49 reference nodes"),
    "limits/7": ("SO,0", 1, 0, 64, "127 reference nodes"),
}
# one scene per family: forced scans over arrays with interior nodes, and the tier kernel with its scene records in LDS
FAMILY_SCENE = {"SO,0": "spheres_plain/1", "SO,1": "spheres_checker/1", "SO,2,uv": "spheres_tex/1", "G,1": "general_plain/1", "G,2,uv": "general_tex/4"}
SCAN_RENDER_SCENES = ("limits/4", "limits/5", "limits/7", "spheres_plain/1")
# The tier kernel's LDS_SCENE = false instantiations: small spheres in their thousands, so that the leaf arrays (2080 bytes per
# slot of 64 leaves) fit the room a tier workgroup has beside a main kernel that keeps nothing in LDS (lds_mode 0) and the
# spheres (32 bytes each) no longer fit beside them.  family: (spheres, with a quad).  Lean families have 158 KB of room, the
# others 52 KB (tier_budget below), hence the two counts.
BIG = {"SO,0": (2600, False), "SO,1": (2600, False), "SO,2,uv": (1500, False), "G,1": (1500, True), "G,2,uv": (1500, True)}
BIG_OPTS = {"lds_mode": 0}


# ------------------------------------------------------------------------------------------------------ the scenes
def load(art, key, nx=NX, ny=NY):
    """Anything with HostScene's surface for a key of SCENES."""
    if "/" in key and key.split("/")[0] in sg.RECIPES:
        recipe, seed = key.split("/")
        return sg.generate(recipe, int(seed), nx, ny)
    if key == "quad_edge":
        return quad_edge_scene(art, nx, ny)
    if key == "bouncing/parallel":                       # as tests/test_carried_constants.py builds it
        import reproject_expect as rx
        from test_carried_constants import _Sky
        cam = art.make_camera((-3.1, 0.12, 13.0), (-3.1, 0.12, 0.0), (0, 1, 0), 0.0, 1.0, 0.0, 13.0, 0.0, 1.0)
        return _Sky(art, rx.WithCamera(art, art.HostScene("bouncing", nx, ny), cam), (0.3, 0.35, 0.5), 1)
    img, iw, ih = art.default_texture(key)
    return art.HostScene(key, nx, ny, img, iw, ih)


def big_scene(family, nx=SNX, ny=SNY):
    """BIG[family]: a ground sphere and a carpet of small ones under twelve shared materials; textured as the family says."""
    count, with_quad = BIG[family]
    rng = np.random.default_rng([99, FAMILIES.index(family)])
    b = sg.Builder(rng)
    level = {"SO,0": 0, "SO,1": 1, "SO,2,uv": 2, "G,1": 1, "G,2,uv": 2}[family]
    if level == 2:
        pool = [b.t_noise(4.0), b.t_image(7, 5), b.t_noodle(1), b.t_uvoff(b.t_image(4, 9), 0.3, -0.2)]
    elif level == 1:
        pool = [b.t_checker(b.t_solid(), b.t_solid(), 0.4) for _ in range(2)]
    else:
        pool = []
    b.leaf(sg._ground(b, pool[0] if pool else -1))
    mats = [b.surface(k, pool) for k in range(12)]
    xs, zs, cell = sg._cells(rng, count)
    r = 0.38 * cell
    for k in range(count):
        b.leaf(b.sphere((xs[k], r, zs[k]), r, mats[k % 12], (0, 0.4 * r, 0) if k % 7 == 3 else (0, 0, 0)))
    if with_quad:
        b.leaf(b.quad((-1.0, 0.0, 3.2), (2.0, 0, 0), (0, 0.8, 0), mats[0]))
    return b.finish(f"big/{family}", sg._camera(rng, nx, ny), nx, ny, ns=2, gradient=1)


def quad_edge_scene(art, nx=NX, ny=NY):
    """A fan of camera rays in the plane y = 0 with a y direction of +0, and an upright quad whose upper edge and whose box's upper
    bound lie in that plane: (bmax.y - origin.y) * (1 / +0) = 0 * inf is a NaN in the box test, which aabb::hit treats as "no
    bound on this axis" (aabb.cuh:45-61: both comparisons with a NaN are false), so the box passes and the ray hits the quad on
    its edge (quad.cuh's interior test includes beta = 1).  A box test that orders the NaN otherwise loses the quad.  Every
    box still contains its object: the description is inside the contract (include/rt_abi.h)."""
    b = sg.Builder(np.random.default_rng([98]))
    b.leaf(b.sphere((0, -200.5, 0), 200.0, b.lambertian()))                       # the ground, half a unit below the fan
    r, lo, hi = b.quad((-0.5, -1.0, 0.0), (1.0, 0, 0), (0, 1.0, 0), b.lambertian())
    hi[1] = 0.0                                                                  # the quad's own upper edge, no padding
    b.leaf((r, lo, hi))
    b.leaf(b.sphere((0.0, 0.3, -3.0), 1.2, b.metal(0.1)))                         # behind the quad: what the rays beside it meet
    b.leaf(b.sphere((0.0, 3.0, 1.0), 0.8, b.light()))
    for k, x in enumerate((-1.4, -0.9, 0.9, 1.4)):
        b.leaf(b.sphere((x, -0.2, 0.8), 0.3, b.surface(k)))
    cam = art.RtCamera()
    cam.origin[:] = (0.0, 0.0, 5.0)
    cam.lower_left_corner[:] = (-1.0, 0.0, 0.0)
    cam.horizontal[:] = (2.0, 0.0, 0.0)
    cam.vertical[:] = (0.0, 0.0, 0.0)
    cam.u[:] = (1.0, 0.0, 0.0)
    cam.v[:] = (0.0, 1.0, 0.0)
    cam.lens_radius, cam.time0, cam.time1 = 0.0, 0.0, 0.0
    return b.finish("quad_edge", cam, nx, ny, gradient=1)


def oracle_of(orc, art, key, scene, nx, ny):
    if key in SCENES and "/" not in key and key != "quad_edge":
        img, iw, ih = art.default_texture(key)
        return orc.OracleScene(key, nx, ny, img, iw, ih)
    return orc.OracleScene.from_host(scene, nx, ny)


# ----------------------------------------------------------------------------- what the library derives from a description
def _array(desc, field, count, dtype):
    n = getattr(desc, count)
    if not n:
        return np.zeros(0, dtype)
    return np.frombuffer((C.c_char * (dtype.itemsize * n)).from_address(getattr(desc, field)), dtype)


def facts(art, scene):
    """spheres_only, tex_level and need_uv as validate() derives them, the family launch_render() picks, and the counts."""
    d = scene.desc
    nodes = _array(d, "nodes", "n_nodes", art.NODE_DTYPE)
    mats = _array(d, "materials", "n_materials", art.MATERIAL_DTYPE)
    kinds = _array(d, "textures", "n_textures", sg.TEXTURE_DTYPE)["kind"]
    prim = nodes["prim"]
    leaves = prim[prim >= 0]
    so = bool(((leaves >> 28) == sg.SPHERE).all()) and not (d.n_quads or d.n_boxes or d.n_instances or d.n_media)
    level = 0
    if (mats["tex"] >= 0).any():                               # as tests/test_aov_host.py derives the level
        level = 1
    if np.isin(kinds, [sg.T_IMAGE, sg.T_NOISE, sg.T_NOODLE, sg.T_FELT, sg.T_UVOFF]).any():
        level = 2
    need_uv = bool(np.isin(kinds, [sg.T_IMAGE, sg.T_UVOFF]).any())
    if so:
        family = ("SO,0", "SO,1", "SO,2,uv")[level]
    else:
        family = "G,1" if level <= 1 and not need_uv else "G,2,uv"
    media_leaves = int(((leaves >> 28) == sg.MEDIUM).sum())
    n_leaves = len(leaves)
    return {"spheres_only": so, "tex_level": level, "need_uv": need_uv, "family": family, "n_leaves": n_leaves, "n_nodes": int(d.n_nodes),
            "n_spheres": int(d.n_spheres), "n_materials": int(d.n_materials), "n_textures": int(d.n_textures), "n_media": int(d.n_media),
            "media_leaves": media_leaves, "tier_data": 0 < n_leaves <= sg.TIER_MAX_LEAVES and media_leaves <= sg.TIER_MAX_MEDIA,
            "n_slots": (n_leaves + 63) // 64}


# ------------------------------------------------------------------ the planning rules, restated (rt_frame_plan.h, rt_device.h)
def main_lds_bytes(mode, n_nodes, f):
    """plan_main_launch: the main kernel's LDS image in a mode -- the walk array with its word table, the spheres, the shade records."""
    image = 32 * n_nodes + ((4 * n_nodes + 15) & ~15)
    return (image if 1 <= mode <= 3 else 0) + (32 * f["n_spheres"] if 2 <= mode <= 3 else 0) + \
           (32 * f["n_materials"] + 64 * f["n_textures"] if mode == 3 else 0)


def mode_fits(mode, n_nodes, f):
    return main_lds_bytes(mode, n_nodes, f) <= LDS_PER_CU - 2048


def expected_mode(lds_mode, scan_nodes, n_nodes, f):
    """plan_main_launch's rule for the staged kernel: a forced mode is taken as it is; otherwise the scan for an array of at most
    scan_nodes nodes, otherwise nodes and spheres in LDS where they fit, else the nodes, else nothing."""
    if lds_mode >= 0:
        return lds_mode
    if scan_nodes > 0 and n_nodes <= scan_nodes:
        return 4
    return 2 if mode_fits(2, n_nodes, f) else 1 if mode_fits(1, n_nodes, f) else 0


def expected_variant(mode, f):
    return 3000 + 100 * mode + 10 * f["tex_level"] + int(f["spheres_only"])


def tier_lds_bytes(n_slots, n_spheres, n_materials, n_textures, scene):
    """rt_tier_lds_bytes: leaf arrays and slot unions, then spheres (32 bytes), materials (32) and textures (64)."""
    b = n_slots * 64 * 32 + n_slots * 32
    if scene:
        b += n_spheres * 32 + n_materials * 32 + n_textures * 64
    return b


def tier_budget(f, main_bytes):
    """plan_frame: the LDS a tier workgroup has beside the main kernel's default workgroup shape.  Lean families (spheres only,
    no noise or image textures): what two 512-thread main workgroups leave over; the others: the slot of one main workgroup
    (three of 256 threads per CU, or one of 768 where the image fits a CU only once), shared by its groups of four waves."""
    lean = f["spheres_only"] and f["tex_level"] < 2
    lds_fit = LDS_PER_CU // (main_bytes + 512) if main_bytes else 8
    per_cu, threads = (2, 512) if lean else (3, 256)
    if lds_fit < per_cu:
        per_cu, threads = 1, (512 if lean else 768)
    if lean:
        used = per_cu * (main_bytes + 512)
        return LDS_PER_CU - used - 1024 if LDS_PER_CU > used + 1024 else 0
    return (LDS_PER_CU // per_cu - 1024) // max(1, threads // 256)


def tier_room(f, main_bytes):
    """plan_tier_room: (fits, lds_scene, lds bytes, tier workgroups per CU of a tail launch)."""
    args = (f["n_slots"], f["n_spheres"], f["n_materials"], f["n_textures"])
    budget = tier_budget(f, main_bytes)
    if not f["tier_data"] or tier_lds_bytes(*args, False) > budget:
        return False, False, 0, 0
    scene = tier_lds_bytes(*args, True) <= budget
    lds = tier_lds_bytes(*args, scene)
    lean = f["spheres_only"] and f["tex_level"] < 2
    return True, scene, lds, max(1, min(LDS_PER_CU // (lds + 512), 4 if lean else 3))


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("key", list(SCENES))
def test_scene_selects_its_family(art, key):
    family, so, level, leaves, _ = SCENES[key]
    s = load(art, key)
    f = facts(art, s)
    assert (f["family"], int(f["spheres_only"]), f["tex_level"], f["n_leaves"]) == (family, so, level, leaves), f
    assert f["n_nodes"] == 2 * leaves - 1, f
    for mode in (0, 1, 2, 3):                                  # every mode fits, with the reference tree itself as the array
        assert mode_fits(mode, f["n_nodes"], f), (mode, f)
    if key.startswith("limits"):
        assert f["n_nodes"] == {"limits/4": 47, "limits/5": 49, "limits/7": 127}[key]
    # the same scene at the schedule's frame size is the same description but for the camera's aspect
    assert facts(art, load(art, key, SNX, SNY)) == f


def test_every_family_has_its_scenes(art):
    assert {SCENES[k][0] for k in SCENES} == set(FAMILIES)
    assert set(FAMILY_SCENE) == set(FAMILIES) and all(SCENES[k][0] == fam for fam, k in FAMILY_SCENE.items())
    # all seven texture kinds in spheres_tex/1; an image with uv in earth, noise in perlin
    def kinds(key):
        s = load(art, key)                                     # (kept alive while its arrays are read)
        return set(_array(s.desc, "textures", "n_textures", sg.TEXTURE_DTYPE)["kind"].tolist())
    assert kinds("spheres_tex/1") == set(range(7))
    assert sg.T_IMAGE in kinds("earth") and sg.T_NOISE in kinds("perlin")
    assert kinds("general_tex/4") == set(range(7)) and kinds("general_tex/3") == set(range(7))
    # every scene of the five has tier data, so that the tier kernel runs for each family
    for fam, key in FAMILY_SCENE.items():
        assert facts(art, load(art, key))["tier_data"], key


def test_general_seeds_have_two_media_and_none(art):
    for recipe in ("general_plain", "general_tex"):
        two, none = {"general_plain": (1, 3), "general_tex": (4, 3)}[recipe]
        assert len(sg.GENERAL_MEDIA[two % len(sg.GENERAL_MEDIA)]) == 2 and len(sg.GENERAL_MEDIA[none % len(sg.GENERAL_MEDIA)]) == 0
        f2, f0 = facts(art, load(art, f"{recipe}/{two}")), facts(art, load(art, f"{recipe}/{none}"))
        assert (f2["n_media"], f2["media_leaves"]) == (2, 2) and (f0["n_media"], f0["media_leaves"]) == (0, 0)
        g = load(art, f"{recipe}/{two}")
        assert set(g.instances()["flags"].tolist()) == {1, 2, 3} and g.desc.n_boxes > 0 and g.desc.n_quads > 6 * g.desc.n_boxes


def test_media_many_has_no_tier_data(art):
    g = load(art, "media_many/0")
    f = facts(art, g)
    assert f["media_leaves"] > 2 and not f["tier_data"] and not g.has_tier_data
    eye = np.array(list(g.desc.camera.origin), np.float64)
    inside = [m for m in g.media() if (m["boundary"] >> 28) == sg.SPHERE and
              np.linalg.norm(g.spheres()[m["boundary"] & 0x0FFFFFFF]["c0"] - eye) < abs(g.spheres()[m["boundary"] & 0x0FFFFFFF]["radius"])]
    assert inside, "the camera sits inside no medium"


def test_zero_direction_cameras(art):
    """Both views have no field of view and no lens, so every camera ray is the one from the eye to the image plane's corner, along
    -z: two zero direction components (bouncing/parallel: far from the origin; degenerate: through it)."""
    # (quad_edge's fan of rays with one zero component has a test of its own below)
    for key, dz in (("bouncing/parallel", -13.0), ("degenerate", -5.0)):
        cam = load(art, key).desc.camera
        assert [abs(x) for x in cam.horizontal] == [0, 0, 0] and [abs(x) for x in cam.vertical] == [0, 0, 0] and cam.lens_radius == 0
        d = np.array(list(cam.lower_left_corner)) - np.array(list(cam.origin))
        assert d.tolist() == [0, 0, dz], (key, d)


def test_quad_edge_rays_meet_a_nan_in_the_box_test_and_hit(art, orc):
    g = load(art, "quad_edge")
    cam, n = g.desc.camera, g.nodes()
    quad_leaf = n[(n["prim"] >> 28 == sg.QUAD) & (n["prim"] >= 0)][0]
    assert quad_leaf["bmax"][1] == 0.0 == cam.origin[1] and quad_leaf["bmin"][1] < -1.0      # 0 * inf on the upper bound only
    s = (np.arange(64, dtype=np.float32) + 0.5) / 64
    d = np.stack([np.float32(-1.0) + s * np.float32(2.0), np.zeros(64, np.float32), np.full(64, -5.0, np.float32)], 1)
    assert not np.signbit(d[:, 1]).any()                                          # + 0: 1 / d.y = + inf
    o = np.tile(np.array([0.0, 0.0, 5.0], np.float32), (64, 1))
    t, p, nrm, uv, mat = orc.OracleScene.from_host(g).trace(o, d, np.zeros(64, np.float32))
    quad_mat = int(g.quads()["mat"][0])
    on_quad = np.abs(d[:, 0]) < 0.5                                               # x at z = 0 is d.x
    assert on_quad.sum() >= 16 and (mat[on_quad] == quad_mat).all() and (t[on_quad] == 1.0).all() and (p[on_quad, 1] == 0.0).all()
    assert (mat[~on_quad] != quad_mat).all() and (mat[~on_quad] >= 0).any()
    assert len(n) <= 24                                                           # scanned by default


@pytest.mark.parametrize("family", FAMILIES)
def test_big_scenes_leave_no_room_for_their_records(art, orc, family):
    """LDS_SCENE = false: beside a main kernel with nothing in LDS the leaf arrays fit a tier workgroup's room, the records do not."""
    g = big_scene(family)
    f = facts(art, g)
    count, with_quad = BIG[family]
    assert f["family"] == family and f["n_leaves"] == count + 1 + int(with_quad) and f["n_spheres"] == count + 1 and f["tier_data"]
    assert f["n_nodes"] > 64                                      # walked, not scanned
    budget = tier_budget(f, main_lds_bytes(BIG_OPTS["lds_mode"], f["n_nodes"], f))
    assert budget == (LDS_PER_CU - 2 * 512 - 1024 if f["spheres_only"] and f["tex_level"] < 2 else LDS_PER_CU // 3 - 1024)
    args = (f["n_slots"], f["n_spheres"], f["n_materials"], f["n_textures"])
    assert tier_lds_bytes(*args, False) <= budget < tier_lds_bytes(*args, True) - 32 * 64     # not by a slot's worth of spheres either
    assert tier_room(f, 0)[:3] == (True, False, f["n_slots"] * 2080)
    # and the scene is worth rendering: rays go on after the first hit, the carpet is seen
    o = orc.OracleScene.from_host(g)
    fb, cnt = o.render(2)
    assert cnt["rays"] >= 1.3 * cnt["samples"] and cnt["sphere_tests"] > 0 and (not with_quad or cnt["quad_tests"] > 0), cnt
    assert not np.isnan(fb).any() and float(fb.std()) > 0.05


def test_family_scenes_keep_their_records_in_lds(art):
    """LDS_SCENE = true: whatever array the planner leaves (its leaves only .. the whole reference tree), in whatever mode."""
    for fam, key in FAMILY_SCENE.items():
        f = facts(art, load(art, key, SNX, SNY))
        for n_nodes in (f["n_leaves"], f["n_nodes"]):
            for mode in (0, 1, 2, 3, 4):
                fits, scene, lds, per_cu = tier_room(f, main_lds_bytes(mode, n_nodes, f))
                assert fits and scene and lds == tier_lds_bytes(f["n_slots"], f["n_spheres"], f["n_materials"], f["n_textures"], True), (key, mode)


def test_restated_rules():
    f = {"n_spheres": 100, "n_materials": 10, "n_textures": 4, "spheres_only": True, "tex_level": 0}
    assert main_lds_bytes(0, 50, f) == 0 == main_lds_bytes(4, 50, f)
    assert main_lds_bytes(1, 50, f) == 50 * 32 + 208 and main_lds_bytes(2, 50, f) == 50 * 32 + 208 + 3200
    assert main_lds_bytes(3, 50, f) == 50 * 32 + 208 + 3200 + 320 + 256
    assert [expected_mode(-1, s, 24, f) for s in (0, 23, 24, 64)] == [2, 2, 4, 4]
    assert [expected_mode(m, 24, 24, f) for m in (0, 1, 2, 3, 4)] == [0, 1, 2, 3, 4]
    assert expected_mode(-1, 24, 6000, dict(f, n_spheres=4096)) == 0 and expected_mode(-1, 24, 4000, dict(f, n_spheres=2400)) == 1
    assert expected_variant(4, dict(f, tex_level=2)) == 3421
    assert tier_lds_bytes(8, 488, 400, 3, False) == 16640 and tier_lds_bytes(1, 2, 3, 4, True) == 2080 + 64 + 96 + 256


def test_tier_room_diagnostic_refuses_bad_arguments(art):
    L = art.rt_lib()
    assert "rt_debug_tier_room" in art.RT_ABI_SYMBOLS and hasattr(L, "rt_debug_tier_room")
    out = (C.c_int32 * 4)(7, 7, 7, 7)
    hip_before = L.rt_last_hip_error()
    assert L.rt_debug_tier_room(None, out) == 1 and "rt_debug_tier_room: null scene" in L.rt_last_error_detail().decode()
    assert L.rt_debug_tier_room(None, None) == 1
    not_a_scene = C.create_string_buffer(1 << 16)               # the output is checked before the scene is looked at
    assert L.rt_debug_tier_room(C.addressof(not_a_scene), None) == 1 and "rt_debug_tier_room: null argument" in L.rt_last_error_detail().decode()
    assert list(out) == [7, 7, 7, 7]
    assert L.rt_last_hip_error() == hip_before                  # refused before any HIP call


def test_creation_options_say_who_reads_them(art):
    L = art.rt_lib()
    try:
        assert L.rt_set_option(b"scan_nodes", 65) == 1
        detail = L.rt_last_error_detail().decode()
        assert "0..64" in detail and "rt_scene_create" in detail and "render" in detail
        assert L.rt_set_option(b"bvh_collapse", 4) == 1 and "rt_scene_create" in L.rt_last_error_detail().decode()
        assert L.rt_set_option(b"lds_mode", 5) == 1 and L.rt_set_option(b"lds_mode", 4) == 0 and L.rt_set_option(b"scan_nodes", 64) == 0
    finally:
        L.rt_reset_options()
