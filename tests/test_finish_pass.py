"""The finishing pass of rt_render and rt_render_window (rt_kernel_finish.hip).

The main kernel and the tier kernel store each finished pixel's colour sum; one elementwise kernel behind the frame's last launch
turns the frame's local rows into store_pixel's values, in place: the scaling by 1 / ns, then gamma by the correctly rounded pow.
Kernel 0 keeps gamma inside the kernel, so on the GPU it is the independent check of the pass; the oracle is the other.

The pass relies on every pixel of the local rows being written exactly once by the frame's last part -- by the main kernel, by
tier 1 or by the tail launch -- and on the sample count being the frame's (a progressive window: the samples so far).  In the
device-buffer cases the caller's buffer is full of NaN before the call: a pixel that no launch wrote stays NaN, and one that was
finished twice is not the oracle's.  (The one pow input that needs the exchange of the rounding test is held by
tests/test_device_math.py through apply_gamma.)
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import assert_frames_equal, render

pytestmark = pytest.mark.gpu

GAMMAS = (1.0, 2.0, 2.2)
# main kernel, tier 1 and tail launch in one frame: a short heavy list whose head goes to the tier kernel, and a hand-off
# threshold of half the frame: the cheap pixels are finished by then, the dear ones have samples left
ALL_WRITERS = {"split_samples": 2, "heavy_factor_x10": 12, "tier1_factor_x10": 20, "tier1_pixels": 64, "tier_auto": 0,
               "handoff_pixels": 2048, "handoff_poll_us": 1}


def _render_into_nan(gpu, hs, frame, opts):
    """The staged kernel into a device buffer filled with NaN; returns (frame as numpy, stats, pixels handed off)."""
    import torch
    L = gpu.rt_lib()
    L.rt_debug_handoff.argtypes = [C.c_void_p, C.c_void_p]
    gpu.reset_options()
    gpu.set_option("kernel", 3)
    for k, v in opts.items():
        gpu.set_option(k, v)
    ds = gpu.DeviceScene(hs)
    try:
        rows = len(gpu.local_rows_to_global(frame))
        buf = torch.full((rows, frame.nx, 3), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _, st = ds.render(frame, out=buf.data_ptr())
        h = np.zeros(2, np.uint64)
        assert L.rt_debug_handoff(ds._p, h.ctypes.data) == 0
        got = buf.cpu().numpy()
    finally:
        ds.close()
        gpu.reset_options()
    return got, st, int(h[0])


@pytest.fixture(scope="module")
def ragged(gpu, orc):
    nx, ny, ns = 37, 19, 3
    hs = gpu.HostScene("bouncing", nx, ny)
    o = orc.OracleScene("bouncing", nx, ny)
    return hs, ns, {g: o.render(ns, gamma=g) for g in GAMMAS}


@pytest.fixture(scope="module")
def square(gpu, orc):
    nx, ny, ns = 64, 64, 8
    hs = gpu.HostScene("bouncing", nx, ny)
    o = orc.OracleScene("bouncing", nx, ny)
    return hs, ns, {g: o.render(ns, gamma=g) for g in GAMMAS}


@pytest.mark.parametrize("gamma", GAMMAS)
def test_unranked_ragged_frame(gpu, ragged, gamma):
    hs, ns, refs = ragged
    ref, cnt = refs[gamma]
    base, st0 = render(gpu, hs, 0, ns=ns, gamma=gamma)
    assert_frames_equal(base, ref, f"kernel 0, gamma {gamma}")
    fb, st, _ = _render_into_nan(gpu, hs, hs.frame(ns=ns, gamma=gamma), {})
    assert st.rays == st0.rays == cnt["rays"]
    assert np.array_equal(fb.view(np.uint32), base.view(np.uint32)), gamma
    assert_frames_equal(fb, ref, f"37x19 into a device buffer, gamma {gamma}")


@pytest.mark.parametrize("gamma", GAMMAS)
def test_ranked_frame_through_main_kernel_tier_and_tail(gpu, square, gamma):
    hs, ns, refs = square
    ref, cnt = refs[gamma]
    base, st0 = render(gpu, hs, 0, ns=ns, gamma=gamma)
    assert_frames_equal(base, ref, f"kernel 0, gamma {gamma}")
    fb, st, handed = _render_into_nan(gpu, hs, hs.frame(ns=ns, gamma=gamma), ALL_WRITERS)
    print("gamma", gamma, "handed off", handed, "of", 64 * 64)
    assert 0 < handed < 64 * 64, handed           # the tail launch finished some pixels, the main kernel others
    assert st.rays == st0.rays == cnt["rays"]
    assert np.array_equal(fb.view(np.uint32), base.view(np.uint32)), gamma
    assert_frames_equal(fb, ref, f"ranked 64x64 into a device buffer, gamma {gamma}")


@pytest.mark.parametrize("gamma", GAMMAS)
def test_row_share_into_its_compact_buffer(gpu, square, gamma):
    hs, ns, refs = square
    ref, _ = refs[gamma]
    f = hs.frame(ns=ns, gamma=gamma, tile_rows=4, tile_first=1, tile_stride=3)
    rows = gpu.local_rows_to_global(f)
    base, st0 = render(gpu, hs, 0, ns=ns, gamma=gamma, tile_rows=4, tile_first=1, tile_stride=3)
    for tag, opts in (("shipped", {}), ("schedule options", ALL_WRITERS)):
        fb, st, _ = _render_into_nan(gpu, hs, f, opts)
        assert fb.shape[0] == len(rows) == st.local_rows > 0
        assert st.rays == st0.rays
        assert np.array_equal(fb.view(np.uint32), base.view(np.uint32)), (tag, gamma)
        assert_frames_equal(fb, ref[rows], f"row share, {tag}, gamma {gamma}")


@pytest.mark.parametrize("gamma", GAMMAS)
def test_progressive_windows_average_over_the_samples_so_far(gpu, orc, square, gamma):
    """Two windows of a frame described with ns = 8: after each the frame is kernel 0's at ns = the window's end."""
    hs, ns, refs = square
    gpu.reset_options()
    ds = gpu.DeviceScene(hs)
    try:
        prog = ds.progressive(hs.frame(ns=ns, gamma=gamma))
        rays = 0
        for begin, end in ((0, 3), (3, ns)):
            fb, st = prog.render(begin, end)
            rays += st.rays
            base, _ = render(gpu, hs, 0, ns=end, gamma=gamma)
            assert np.array_equal(fb.view(np.uint32), base.view(np.uint32)), (gamma, begin, end)
        prog.close()
    finally:
        ds.close()
    ref, cnt = refs[gamma]
    assert rays == cnt["rays"]
    assert_frames_equal(fb, ref, f"two windows, gamma {gamma}")


@pytest.mark.parametrize("gamma", GAMMAS)
def test_host_buffer_path(gpu, square, gamma):
    """A host buffer: the pass runs on the library's own device frame before the copy back."""
    hs, ns, refs = square
    ref, cnt = refs[gamma]
    for opts in ({}, ALL_WRITERS):
        fb, st = render(gpu, hs, 3, opts, ns=ns, gamma=gamma)
        assert st.rays == cnt["rays"]
        assert_frames_equal(fb, ref, f"host buffer, gamma {gamma}, {opts}")
