"""The main kernel's stop / resume path and its "a leaf is noted" bookkeeping (rt_kernel_staged.h, stage A and stage B).

With its nodes in LDS (lds_mode 1, 2, 3) the box step writes two things only: `pend`, the first leaf whose box passed, and
`node`.  Whether a leaf is noted is read out of `pend` in every step of every trip (one comparison together with "the record
is an interior node"), and a lane that passes a second leaf while the first is still due stops with node = the leaf's link
word, which in the LDS image is ~(the leaf record's own address).  Stage B takes everything else from that: the stopped-at
record (~node), its object reference (the word table staged behind the image, one word a record) and the way on (that
record's skip link), and the stopped-at leaf becomes the noted one once the noted one is tested.

Each frame here must be kernel 0's and the oracle's bit for bit with equal ray counts, in the smallest scenes where that
path can go wrong and with trips cut so that lanes stop, wait and resume, are noted in one half of an unrolled step pair and
stopped in the other, and carry a noted leaf from one trip into the next.
"""
import numpy as np
import pytest

from test_desc_oracle import NS, NX, NY
from test_gpu_parity import assert_frames_equal, render
from test_walk_links import _device_nodes, _one_object_scene

pytestmark = pytest.mark.gpu

# scene: frame, and the LDS modes it can take (crowd_2400: its walk array fits a CU's LDS, its spheres beside it do not)
FRAME_CASES = {"two_spheres": (16, 8, 4, (1, 2, 3)),           # the smallest tree
               "one_object": (NX, NY, NS, (1, 2, 3)),          # the root is a leaf: a stopped lane resumes at the array's end
               "degenerate": (32, 16, 8, (1, 2, 3)),           # rays with a zero direction component: the reference-form trip
               "crowd_2400": (48, 32, 2, (1,)),                # overlapping leaves: many second leaves
               "instanced": (48, 48, 4, (1, 2, 3)),            # general families: the kind bits of RT_PRIM_REF through the table
               "fog": (48, 48, 4, (1, 2, 3))}                  # ... media too; forced off the scan
OPTION_SETS = ({},                                             # the shipped trip
               {"steps_per_trip": 1, "leaf_threshold": 64},    # lanes stop at a second leaf, wait, resume with it noted
               {"steps_per_trip": 1, "leaf_threshold": 1},     # every noted leaf is tested at once
               {"steps_per_trip": 12, "leaf_threshold": 64},   # noted in one half of an unrolled pair, stopped in the other
               {"steps_per_trip": 3, "leaf_threshold": 64})    # an odd trip: a noted leaf is carried into the next one


@pytest.mark.parametrize("name", list(FRAME_CASES))
def test_stopped_lanes_resume_in_every_lds_mode(gpu, orc, name):
    nx, ny, ns, modes = FRAME_CASES[name]
    assert nx <= 64 and ny <= 48 and ns <= 8
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


def test_book2_final_image_with_its_table_fits(gpu, orc):
    """Book-2 final, the largest built-in walk array, in the mode the library chooses for it: the image is the node records
    plus one word a record (padded to 16 bytes), it still goes to LDS, and the frame is the oracle's."""
    name, nx, ny, ns = "final", 32, 32, 2
    img, iw, ih = gpu.default_texture(name)
    hs = gpu.HostScene(name, nx, ny, img, iw, ih)
    ref, cnt = orc.OracleScene(name, nx, ny, img, iw, ih).render(ns)
    gpu.reset_options()
    ds = gpu.DeviceScene(hs)
    try:
        n_nodes = len(_device_nodes(gpu, ds, 1))
    finally:
        ds.close()
    fb, st = render(gpu, hs, 3, ns=ns)
    mode = st.kernel_variant // 100 % 10
    image = 32 * n_nodes + ((4 * n_nodes + 15) & ~15)
    print("final: walk nodes", n_nodes, "lds_mode", mode, "lds_bytes", st.lds_bytes, "image", image)
    assert st.kernel_variant // 1000 == 3 and mode in (1, 2, 3), st.kernel_variant
    assert n_nodes > 2048                      # an image past 64 KB, one workgroup a CU
    assert st.lds_bytes == image if mode == 1 else st.lds_bytes > image, (st.lds_bytes, image)
    assert st.lds_bytes <= 160 * 1024
    assert st.rays == cnt["rays"], (st.rays, cnt["rays"])
    assert_frames_equal(fb, ref, "final, shipped lds_mode")
