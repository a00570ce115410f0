"""Where the main kernel adds the background term of a path that ends in a miss (rt_kernel_staged.h, after stage B and stage E).

A lane whose walk finishes with no hit goes to the path-end state at once and only marks that its path ended in a miss (a
negative `bounce`); stage E, which runs when enough lanes wait for it, adds throughput * miss_color(ray) to the path's radiance
as its first act, before the sample is added to the pixel and before the pixel is stored, parked or handed off.  The ray, the
throughput and the radiance are the ones the lane had when it missed, so frames and ray counts are what they were.

What can go wrong: a path end that is no miss gets the term (emission, an absorbed metal scatter, the 50-bounce cut, a lane that
starts or turns ordinary with no path behind it), or a miss loses it (the pixel parked or handed off before the term is added, a
lane left waiting while other stages run around it).  Each frame here must be kernel 0's and the oracle's bit for bit with equal
ray counts, on scenes whose paths end in each of those ways, in every LDS mode the scene can take, with the stage quorums and
the hand-off set so that missed lanes wait, go at once, or park at once.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import assert_frames_equal, render

pytestmark = pytest.mark.gpu

NX, NY, NS = 64, 64, 8   # 64 work tiles: the smallest frame the cost-aware schedule splits

# scene: what its paths end in, and the LDS modes it is forced into (None: the library's choice)
SCENES = {"book1": (None, 0, 1, 2, 3),           # gradient sky, metal (absorbed scatters) and glass
          "bouncing": (None, 0, 1, 2, 3),        # the headline's scene: metal, glass, emitters, a solid background (the term without its gradient)
          "cornell": (None, 0, 1, 2, 3),         # a closed box: the light or 50 bounces, never the sky; the library's choice is the scan (4)
          "simple_light": (None, 0, 1, 2, 3),    # solid background, emitters
          "degenerate": (None, 0, 1, 2, 3)}      # rays with a zero direction component: the reference-form trip
RANKED = {"heavy_factor_x10": 12, "sparse_factor_x10": 20, "tier1_factor_x10": 30, "tier1_pixels": 64}
OPTION_SETS = (("shipped", {}),
               ("missed lanes wait", {"newpath_threshold": 64}),           # ... while stages C, D and F run around them
               ("missed lanes go at once", {"newpath_threshold": 1}),
               ("one step a trip", {"steps_per_trip": 1}),
               # every pixel leaves for the tail launch after its first sample: a missed lane parks at once
               ("handed off", dict(RANKED, split_samples=4, handoff_pixels=1 << 24, handoff_poll_us=1)),
               # parts, tiers, sparse and semi waves; waves that turn ordinary
               ("split", dict(RANKED, split_samples=2, presplit_samples=1, semi_stride=4, sparse_stride=8)))


def _render(gpu, hs, opts, ns):
    """render() of test_gpu_parity with the staged kernel, plus how many pixels the frame handed off."""
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
        fb, st = ds.render(hs.frame(ns=ns))
        h = np.zeros(2, np.uint64)
        assert L.rt_debug_handoff(ds._p, h.ctypes.data) == 0
    finally:
        ds.close()
        gpu.reset_options()
    return fb, st, int(h[0])


@pytest.mark.parametrize("name", list(SCENES))
def test_miss_term_is_added_once_where_the_path_ends(gpu, orc, name):
    img, iw, ih = gpu.default_texture(name)
    hs = gpu.HostScene(name, NX, NY, img, iw, ih)
    ref, cnt = orc.OracleScene(name, NX, NY, img, iw, ih).render(NS)
    base, st0 = render(gpu, hs, 0, ns=NS)
    assert st0.rays == cnt["rays"], (name, st0.rays, cnt["rays"])
    assert_frames_equal(base, ref, f"{name} kernel 0")
    modes_seen = set()
    for mode in SCENES[name]:
        for tag, opts in OPTION_SETS:
            fb, st, handed = _render(gpu, hs, opts if mode is None else dict(opts, lds_mode=mode), NS)
            what = f"{name} lds_mode {mode}: {tag}"
            got_mode = st.kernel_variant // 100 % 10
            assert st.kernel_variant // 1000 == 3 and (mode is None or got_mode == mode), (what, st.kernel_variant)
            modes_seen.add(got_mode)
            print(what, "variant", st.kernel_variant, "rays", st.rays, "handed off", handed)
            assert st.rays == st0.rays == cnt["rays"], (what, st.rays, st0.rays, cnt["rays"])
            assert np.array_equal(fb.view(np.uint32), base.view(np.uint32)), what
            assert_frames_equal(fb, ref, what)
            if tag == "handed off" and mode is None and name != "degenerate":
                assert handed > 0, what          # the path under test did run (as in test_tail_handoff_matches_oracle)
    assert modes_seen >= {0, 1, 2, 3}, modes_seen
    if name == "cornell":
        assert 4 in modes_seen, modes_seen       # the scan form of the trip
