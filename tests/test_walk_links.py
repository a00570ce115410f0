"""The main kernel's walk-private link encoding (rt_kernel_staged.h, stage_scene<.., true>).

With its node array in LDS (lds_mode 1, 2, 3) the main kernel walks LDS addresses over an image whose two link words it
re-encoded while staging; with the nodes in global memory (lds_mode 0) or scanned (4) it walks node indices over the device
arrays as they are.  Both forms must give kernel 0's and the oracle's frame bit for bit, with equal ray counts, whatever the
trip length and the leaf quorum -- including lanes that stop at a second leaf while the first is still due and resume from
the parked record's skip link.  The device arrays themselves keep their documented encoding (rt_debug_scene_boxes).
"""
import ctypes as C

import numpy as np
import pytest

import scene_gen as sg
from test_desc_oracle import NS, NX, NY
from test_gpu_parity import assert_frames_equal, render

pytestmark = pytest.mark.gpu

LEAF_SKIP_SCENES = ["two_spheres", "bouncing", "degenerate", "cornell", "cornell_smoke", "final", "instanced", "fog", "crowd_2400"]


def _device_nodes(art, ds, which):
    """rt_debug_scene_boxes: node array `which` (0 the reference's tree, 1 the walk array) in the device's link encoding."""
    n = C.c_size_t(0)
    assert art.rt_lib().rt_debug_scene_boxes(ds._p, which, None, 0, C.byref(n)) == 0
    out = np.zeros(n.value // art.NODE_DTYPE.itemsize, art.NODE_DTYPE)
    if n.value:
        assert art.rt_lib().rt_debug_scene_boxes(ds._p, which, out.ctypes.data, out.nbytes, C.byref(n)) == 0
    return out


@pytest.mark.parametrize("name", LEAF_SKIP_SCENES)
def test_every_leaf_skips_to_the_next_record(gpu, name):
    """Both node arrays are depth-first: a leaf's decoded skip link is its own index + 1, an interior node's decoded prim
    too, and every skip link moves forward and stays inside the array -- what the LDS image's addresses are built from."""
    img, iw, ih = gpu.default_texture(name)
    hs = gpu.HostScene(name, 32, 32, img, iw, ih)
    gpu.reset_options()
    ds = gpu.DeviceScene(hs)
    try:
        arrays = [_device_nodes(gpu, ds, which) for which in (0, 1)]
    finally:
        ds.close()
    for which, n in enumerate(arrays):
        assert len(n) > 0, (name, which)
        idx = np.arange(len(n), dtype=np.int64)
        skip = ~n["skip"].astype(np.int64)
        leaf = n["prim"] >= 0
        assert leaf.any()
        assert np.array_equal(skip[leaf], idx[leaf] + 1), (name, which, np.flatnonzero(skip[leaf] != idx[leaf] + 1)[:5])
        assert np.array_equal(~n["prim"][~leaf].astype(np.int64), idx[~leaf] + 1), (name, which)
        assert (skip > idx).all() and (skip <= len(n)).all(), (name, which)
    print(name, "reference nodes", len(arrays[0]), "walk nodes", len(arrays[1]))


def _one_object_scene(art):
    """A description whose root is a leaf (one sphere): the walk's first record is its last, and a lane that stops there
    resumes at the end of the array."""
    g = sg.generate("spheres_plain", 1)
    n = g.nodes()
    leaves = n[n["prim"] >= 0]
    one = np.zeros(1, art.NODE_DTYPE)
    one[0] = leaves[len(leaves) // 2]
    one["skip"][0] = 1
    return sg.GenScene("one_object", dict(g._a, nodes=one), g.desc.camera, NX, NY, NS, g.gamma, g.background, g.use_gradient_bg, ())


# scene: frame, and the LDS modes it can take (crowd_2400: its walk array fits a CU's LDS, its spheres beside it do not)
FRAME_CASES = {"two_spheres": (16, 8, 4, (0, 1, 2, 3)),          # the smallest tree
               "one_object": (NX, NY, NS, (0, 1, 2, 3)),         # the root is a leaf
               "bouncing": (64, 40, 6, (0, 1, 2, 3)),
               "degenerate": (32, 16, 8, (0, 1, 2, 3)),          # rays with a zero direction component: the reference-form trip
               "cornell": (48, 48, 4, (0, 1, 2, 3)),             # forced off the scan: quads and boxes decoded from the image
               "fog": (48, 48, 4, (0, 1, 2, 3)),                 # ... and media
               "instanced": (48, 48, 4, (0, 1, 2, 3)),
               "crowd_2400": (48, 32, 2, (0, 1))}                # overlapping leaves
# the shipped trip; lanes stop at a second leaf while the first is due, and resume; every noted leaf is tested at once
OPTION_SETS = ({}, {"steps_per_trip": 1, "leaf_threshold": 64}, {"leaf_threshold": 1})


@pytest.mark.parametrize("name", list(FRAME_CASES))
def test_frames_are_the_same_in_every_lds_mode(gpu, orc, name):
    nx, ny, ns, modes = FRAME_CASES[name]
    if name == "one_object":
        hs = _one_object_scene(gpu)
        ref, cnt = orc.OracleScene.from_host(hs).render(ns)
    else:
        img, iw, ih = gpu.default_texture(name)
        hs = gpu.HostScene(name, nx, ny, img, iw, ih)
        ref, cnt = orc.OracleScene(name, nx, ny, img, iw, ih).render(ns)
    base, st0 = render(gpu, hs, 0, ns=ns)
    assert st0.rays == cnt["rays"], (name, st0.rays, cnt["rays"])
    assert_frames_equal(base, ref, f"{name} kernel 0")
    for mode in modes:
        for opts in OPTION_SETS:
            fb, st = render(gpu, hs, 3, dict(opts, lds_mode=mode), ns=ns)
            what = f"{name} lds_mode {mode} {opts}"
            assert st.kernel_variant // 1000 == 3 and st.kernel_variant // 100 % 10 == mode, (what, st.kernel_variant)
            assert st.rays == st0.rays == cnt["rays"], (what, st.rays, st0.rays, cnt["rays"])
            assert np.array_equal(fb.view(np.uint32), base.view(np.uint32)), what
            assert_frames_equal(fb, ref, what)
