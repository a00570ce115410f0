"""Values the lean main kernels keep or fetch at another moment than before (rt_kernel_staged.h, RT_CARRY_LOOSE and RT_KERNARG_AT_USE).

The walk loop's addends (LooseRay) are written in stage F with the ray's 1/d and kept until the ray's next stage F, instead of being
computed in every trip's prologue; stage E reads the camera record and the miss term's background from the kernel-argument segment
where it uses them.  Neither changes a value, so every frame here must be kernel 0's and the oracle's bit for bit with equal ray
counts.

What can go wrong with the addends: a lane walks with the previous ray's.  So: scenes with many rays per pixel and rays that end
in every way, rays with a zero direction component beside finite ones in one wave (`degenerate`), a general scene forced off the
scan, a crowd of overlapping leaves; every LDS mode the scene can take (address form and index form of the walk); many trips on
one set of addends (`steps_per_trip` 1); stage F run for one lane or for many at once (the quorums of stages C and E at 1 and 64);
waves that turn ordinary, pixels parked, resumed and handed off.

What can go wrong with the reads: a wrong offset, or a record that is not this launch's.  So: a camera with lens and shutter, a
pinhole, a camera replaced on a resident scene and put back; a gradient sky and a solid, non-black background; a row share
and a frame that is not square (the fields that lie beside the background in the block).
"""
import numpy as np
import pytest

import reproject_expect as rx
from test_gpu_parity import assert_frames_equal, render
from test_path_end import RANKED, _render

pytestmark = pytest.mark.gpu

NX, NY, NS = 64, 64, 8   # 64 work tiles: the smallest frame the cost-aware schedule splits

# scene: the LDS modes it is forced into (crowd_2400: its walk array fits a CU's LDS, its spheres beside it do not)
WALK_SCENES = {"bouncing": (0, 1, 2, 3),       # the headline's scene: metal, glass, emitters, moving spheres
               "book1": (0, 1, 2, 3),          # gradient sky, metal and glass
               "degenerate": (0, 1, 2, 3),     # rays with a zero direction component beside finite ones: both trips in one wave
               "cornell": (0, 1, 2, 3),        # forced off the scan: the general family's per-trip form
               "crowd_2400": (0, 1),           # 2 400 overlapping spheres: long walks, many leaves noted
               # the headline's scene under a sky, seen through parallel rays along -z (a field of view of 0, no lens): every camera ray has
               # two zero direction components and every ray after it none, so each finite ray of a lane follows one that
               # was not, far from the origin (`degenerate`'s first bounce starts at the origin itself, where stale addends
               # are nearly right)
               "bouncing/parallel": (0, 1, 2, 3)}
OPTION_SETS = (("shipped", {}),
               ("one step a trip", {"steps_per_trip": 1}),                # many trips per ray on one set of addends
               ("stage E for one lane", {"newpath_threshold": 1}),       # ... so stage F runs for one lane
               ("stage E for all", {"newpath_threshold": 64}),           # ... or for many at once
               ("stage C for one lane", {"shade_threshold": 1}),
               ("stage C for all", {"shade_threshold": 64}),
               ("handed off", dict(RANKED, split_samples=4, handoff_pixels=1 << 24, handoff_poll_us=1)),
               ("split", dict(RANKED, split_samples=2, presplit_samples=1, semi_stride=4, sparse_stride=8)))
DEGREES = 20.0
EYE = (13.0, 2.0, 3.0)   # host/rtw_scenes.cpp, bouncing_spheres


class _Sky:
    """A scene under another background: the same description, other frame defaults."""

    def __init__(self, art, scene, background, gradient):
        self._w = rx.WithCamera(art, scene, scene.desc.camera)
        self.name, self.desc = scene.name + "/sky", self._w.desc
        self.nx, self.ny, self.ns, self.gamma = scene.nx, scene.ny, scene.ns, scene.gamma
        self.background, self.use_gradient_bg = [float(x) for x in background], int(gradient)
        self.materials = scene.materials
        self.frame = lambda **kw: art.HostScene.frame(self, **kw)


def _check(gpu, hs, ref, rays, modes, option_sets, what, **frame_kw):
    """Kernel 0 against the oracle, then the main kernel in every mode and option set against both."""
    base, st0 = render(gpu, hs, 0, ns=NS, **frame_kw)
    assert st0.rays == rays, (what, st0.rays, rays)
    assert_frames_equal(base, ref, f"{what} kernel 0")
    for mode in modes:
        for tag, opts in option_sets:
            o = dict(opts) if mode is None else dict(opts, lds_mode=mode)
            if frame_kw:
                fb, st = render(gpu, hs, 3, o, ns=NS, **frame_kw)
            else:
                fb, st, _ = _render(gpu, hs, o, NS)
            w = f"{what} lds_mode {mode}: {tag}"
            assert st.kernel_variant // 1000 == 3 and (mode is None or st.kernel_variant // 100 % 10 == mode), (w, st.kernel_variant)
            assert st.rays == st0.rays == rays, (w, st.rays, st0.rays, rays)
            assert np.array_equal(fb.view(np.uint32), base.view(np.uint32)), w
            assert_frames_equal(fb, ref, w)


@pytest.mark.parametrize("name", list(WALK_SCENES))
def test_every_ray_walks_with_its_own_addends(gpu, orc, name):
    if name == "bouncing/parallel":
        cam = gpu.make_camera((-3.1, 0.12, 13.0), (-3.1, 0.12, 0.0), (0, 1, 0), 0.0, 1.0, 0.0, 13.0, 0.0, 1.0)
        assert list(cam.horizontal) == [0, 0, 0] and list(cam.vertical) == [0, 0, 0] and cam.lens_radius == 0
        hs = _Sky(gpu, rx.WithCamera(gpu, gpu.HostScene("bouncing", NX, NY), cam), (0.3, 0.35, 0.5), 1)
        ref, cnt = orc.OracleScene.from_host(hs, NX, NY).render(NS)
        assert cnt["rays"] > 3 * NX * NY * NS and float(ref.std()) > 0.1   # the parallel rays hit something diffuse and go on, to the sky
    else:
        img, iw, ih = gpu.default_texture(name)
        hs = gpu.HostScene(name, NX, NY, img, iw, ih)
        ref, cnt = orc.OracleScene(name, NX, NY, img, iw, ih).render(NS)
    _check(gpu, hs, ref, cnt["rays"], WALK_SCENES[name], OPTION_SETS, name)


def _orbited(gpu, nx, ny, aperture):
    return gpu.make_camera(rx.orbit(EYE, (0, 0, 0), DEGREES), (0, 0, 0), (0, 1, 0), 30.0, nx / ny, aperture, float(np.linalg.norm(EYE)), 0.0, 1.0)


@pytest.mark.parametrize("mode", [None, 0, 1, 2, 3])
def test_the_camera_read_is_the_launchs_own(gpu, orc, mode):
    """One resident scene (lens and shutter), its camera replaced by a view 20 degrees away and put back: each frame is a fresh
    scene's and the oracle's."""
    hs = gpu.HostScene("bouncing", NX, NY)
    cam = _orbited(gpu, NX, NY, 0.1)
    assert hs.desc.camera.lens_radius > 0 and hs.desc.camera.time1 > hs.desc.camera.time0
    moved = rx.WithCamera(gpu, hs, cam)
    views = []
    for scene in (hs, moved):
        ref, cnt = orc.OracleScene.from_host(scene, NX, NY).render(NS)
        fresh, st = render(gpu, scene, 3, None if mode is None else {"lds_mode": mode}, ns=NS)
        assert st.rays == cnt["rays"]
        assert_frames_equal(fresh, ref, f"{scene.name} fresh, lds_mode {mode}")
        views.append((ref, cnt["rays"], fresh))
    assert not np.array_equal(views[0][0], views[1][0])                 # another view, not the same frame again
    gpu.reset_options()
    gpu.set_option("kernel", 3)
    if mode is not None:
        gpu.set_option("lds_mode", mode)
    ds = gpu.DeviceScene(hs)
    try:
        for step, (camera, view) in enumerate(((None, 0), (cam, 1), (hs.desc.camera, 0), (cam, 1))):
            if camera is not None:
                ds.set_camera(camera)
            fb, st = ds.render(hs.frame(ns=NS))
            ref, rays, fresh = views[view]
            what = f"resident scene, step {step}, lds_mode {mode}"
            assert st.kernel_variant // 1000 == 3 and (mode is None or st.kernel_variant // 100 % 10 == mode), (what, st.kernel_variant)
            assert st.rays == rays, (what, st.rays, rays)
            assert np.array_equal(fb.view(np.uint32), fresh.view(np.uint32)), what
            assert_frames_equal(fb, ref, what)
    finally:
        ds.close()
        gpu.reset_options()


FRAMES = {"pinhole": dict(aperture=0.0),
          "solid background": dict(sky=((0.3, 0.35, 0.5), 0)),
          "solid background behind a pinhole": dict(aperture=0.0, sky=((0.7, 0.2, 0.05), 0)),
          "gradient sky": dict(sky=((0.3, 0.35, 0.5), 1)),             # (the solid colour beside it must not show)
          "row share": dict(sky=((0.3, 0.35, 0.5), 0), frame=dict(tile_rows=4, tile_first=1, tile_stride=2)),
          "96 x 40": dict(sky=((0.3, 0.35, 0.5), 1), size=(96, 40))}


@pytest.mark.parametrize("case", list(FRAMES))
def test_records_read_in_stage_e(gpu, orc, case):
    c = FRAMES[case]
    nx, ny = c.get("size", (NX, NY))
    hs = gpu.HostScene("bouncing", nx, ny)
    if "aperture" in c:
        hs = rx.WithCamera(gpu, hs, _orbited(gpu, nx, ny, c["aperture"]))
        assert hs.desc.camera.lens_radius == 0.0
    if "sky" in c:
        hs = _Sky(gpu, hs, *c["sky"])
    o = orc.OracleScene.from_host(hs, nx, ny)
    ref, cnt = o.render(NS)
    rays = cnt["rays"]
    kw = c.get("frame", {})
    if kw:
        rows = gpu.local_rows_to_global(hs.frame(ns=NS, **kw))
        assert 0 < len(rows) < ny and len(rows) % kw["tile_rows"] == 0
        ref = ref[rows]
        # the share's rays: the oracle's count over each of its row bands
        rays = sum(o.render(NS, row0=int(r), row1=int(r) + kw["tile_rows"])[1]["rays"] for r in rows[::kw["tile_rows"]])
    if "sky" in c:
        assert float(ref.max()) > 0.2                                    # the background does reach the frame
    _check(gpu, hs, ref, rays, (None, 0, 1, 2, 3), OPTION_SETS[:1] + OPTION_SETS[-2:], case, **kw)
