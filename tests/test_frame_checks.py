"""The frame checks of every entry point that takes a frame description, pinned word for word.

The entries share one check (check_frame, csrc/rt_host.h) but keep their own texts, which the Python layer and other tests
match on.  EXPECT_HOST and EXPECT_DEVICE hold the (status, detail) each entry returned for each bad frame BEFORE the checks
were shared, recorded from that build, with three additions.  All three concern the frame that has fewer than 2^31 pixels but
2^31 work items in its 8x8 tiles (1 x 2^28):
  * rt_progressive_state_create accepted it (rt_render_window would then have refused the state's frame) and now returns
    RT_ERR_INVALID "bad frame size";
  * rt_debug_prior accepted it too (and would have needed 10 GB for it) and now returns "rt_debug_prior: bad frame size";
  * rt_render_adaptive refused it with the text below, but only after it had made the scene's device current and grown the
    scene's buffers, so that build could not be asked without a scene; the check now comes with the other three.

The host part runs without a device: the scene pointer is fake and never dereferenced, because every check here fails before
the scene or any HIP call is touched.  46000 x 46000 is NOT a frame with too many tiles -- 5750^2 tiles x 64 = 2 116 000 000
< 2^31 -- and passes every check, so only the two entries that look for a null scene after the frame checks are given it, with
a null scene: it must get that far.  The device part makes one tiny scene and renders nothing."""
import ctypes as C

import numpy as np
import pytest

OK, INVALID = 0, 1
FAKE = 0x1000   # never dereferenced
BIG_ROWS = 1 << 28   # 1 x 2^28 pixels in one tile row-block: 2^25 tiles x 64 = 2^31 work items

BAD_FRAMES = {
    "zero width": dict(nx=0),
    "negative height": dict(ny=-4),
    "2^31 pixels": dict(nx=1 << 16, ny=1 << 15),
    "ns = 0": dict(ns=0),
    "tile count overflow": dict(nx=1, ny=BIG_ROWS, tile_rows=BIG_ROWS),
    "tile_rows = 0": dict(tile_rows=0),
    "tile_stride = 0": dict(tile_stride=0),
    "tile_first = -1": dict(tile_first=-1),
}

EXPECT_HOST = {
    "rt_render_adaptive": {
        "zero width": (INVALID, "rt_render_adaptive: bad frame size"),
        "negative height": (INVALID, "rt_render_adaptive: bad frame size"),
        "2^31 pixels": (INVALID, "rt_render_adaptive: bad frame size"),
        "tile count overflow": (INVALID, "rt_render_adaptive: frame too large"),
        "tile_rows = 0": (INVALID, "rt_render_adaptive: bad row partition"),
        "tile_stride = 0": (INVALID, "rt_render_adaptive: bad row partition"),
        "tile_first = -1": (INVALID, "rt_render_adaptive: bad row partition"),
    },
    "rt_render_variance": {
        "zero width": (INVALID, "rt_render_variance: bad frame size"),
        "negative height": (INVALID, "rt_render_variance: bad frame size"),
        "2^31 pixels": (INVALID, "rt_render_variance: bad frame size"),
        "ns = 0": (INVALID, "rt_render_variance: ns must be a positive multiple of batches"),
        "tile count overflow": (INVALID, "rt_render_variance: bad frame size (too many 8x8 tiles)"),
        "tile_rows = 0": (INVALID, "rt_render_variance: bad row partition"),
        "tile_stride = 0": (INVALID, "rt_render_variance: bad row partition"),
        "tile_first = -1": (INVALID, "rt_render_variance: bad row partition"),
    },
    "rt_render_aov": {
        "zero width": (INVALID, "rt_render_aov: nx, ny and ns must be positive"),
        "negative height": (INVALID, "rt_render_aov: nx, ny and ns must be positive"),
        "2^31 pixels": (INVALID, "rt_render_aov: frame too large"),
        "ns = 0": (INVALID, "rt_render_aov: nx, ny and ns must be positive"),
        "tile count overflow": (INVALID, "rt_render_aov: frame too large"),
        "tile_rows = 0": (INVALID, "rt_render_aov: bad row partition"),
        "tile_stride = 0": (INVALID, "rt_render_aov: bad row partition"),
        "tile_first = -1": (INVALID, "rt_render_aov: bad row partition"),
        "46000 x 46000, null scene": (INVALID, "rt_render_aov: null scene"),
    },
    "rt_render_aov_through": {
        "zero width": (INVALID, "rt_render_aov_through: nx, ny and ns must be positive"),
        "negative height": (INVALID, "rt_render_aov_through: nx, ny and ns must be positive"),
        "2^31 pixels": (INVALID, "rt_render_aov_through: frame too large"),
        "ns = 0": (INVALID, "rt_render_aov_through: nx, ny and ns must be positive"),
        "tile count overflow": (INVALID, "rt_render_aov_through: frame too large"),
        "tile_rows = 0": (INVALID, "rt_render_aov_through: bad row partition"),
        "tile_stride = 0": (INVALID, "rt_render_aov_through: bad row partition"),
        "tile_first = -1": (INVALID, "rt_render_aov_through: bad row partition"),
        "46000 x 46000, null scene": (INVALID, "rt_render_aov_through: null scene"),
    },
}
EXPECT_DEVICE = {
    "rt_render": {
        "zero width": (INVALID, "nx, ny and ns must be positive"),
        "negative height": (INVALID, "nx, ny and ns must be positive"),
        "2^31 pixels": (INVALID, "frame too large"),
        "ns = 0": (INVALID, "nx, ny and ns must be positive"),
        "tile count overflow": (INVALID, "frame too large"),
        "tile_rows = 0": (INVALID, "bad row partition"),
        "tile_stride = 0": (INVALID, "bad row partition"),
        "tile_first = -1": (INVALID, "bad row partition"),
    },
    "rt_render_window": {
        "zero width": (INVALID, "rt_render_window: the frame description differs from the one the state was created for"),
        "negative height": (INVALID, "rt_render_window: the frame description differs from the one the state was created for"),
        "2^31 pixels": (INVALID, "rt_render_window: the frame description differs from the one the state was created for"),
        "tile count overflow": (INVALID, "rt_render_window: the frame description differs from the one the state was created for"),
        "tile_rows = 0": (INVALID, "rt_render_window: the frame description differs from the one the state was created for"),
        "tile_stride = 0": (INVALID, "rt_render_window: the frame description differs from the one the state was created for"),
        "tile_first = -1": (INVALID, "rt_render_window: the frame description differs from the one the state was created for"),
    },
    "rt_progressive_state_create": {
        "zero width": (INVALID, "bad frame size"),
        "negative height": (INVALID, "bad frame size"),
        "2^31 pixels": (INVALID, "bad frame size"),
        "ns = 0": (OK, ""),
        "tile count overflow": (INVALID, "bad frame size"),
        "tile_rows = 0": (INVALID, "bad row partition"),
        "tile_stride = 0": (INVALID, "bad row partition"),
        "tile_first = -1": (INVALID, "bad row partition"),
    },
    "rt_debug_prior": {
        "zero width": (INVALID, "rt_debug_prior: bad frame size"),
        "negative height": (INVALID, "rt_debug_prior: bad frame size"),
        "2^31 pixels": (INVALID, "rt_debug_prior: bad frame size"),
        "tile count overflow": (INVALID, "rt_debug_prior: bad frame size"),
        "tile_rows = 0": (INVALID, "rt_debug_prior: bad row partition"),
        "tile_stride = 0": (INVALID, "rt_debug_prior: bad row partition"),
        "tile_first = -1": (INVALID, "rt_debug_prior: bad row partition"),
    },
}


def frame(art, **kw):
    f = art.RtFrameDesc()
    f.nx, f.ny, f.ns, f.gamma = 8, 8, 2, 1.0
    f.tile_rows, f.tile_first, f.tile_stride = 8, 0, 1
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _result(art, st):
    return st, art.rt_lib().rt_last_error_detail().decode() if st != OK else ""   # (the detail of a call that succeeded is an earlier call's)


# ---- the entries that check the frame before the scene is looked at (a fake scene pointer, no device)
def call_adaptive(art, f, scene=FAKE):
    a = art.RtAdaptiveDesc(4, 16, 0.1, 0.01)
    return _result(art, art.rt_lib().rt_render_adaptive(scene, C.byref(f), C.byref(a), FAKE, 1, None, None, None))


def call_variance(art, f, scene=FAKE):
    v = art.RtVarianceDesc(2, 0)
    return _result(art, art.rt_lib().rt_render_variance(scene, C.byref(f), C.byref(v), FAKE, 1, FAKE, None, None))


def call_aov(art, f, scene=FAKE):
    a = art.RtAovDesc()
    a.albedo = FAKE
    return _result(art, art.rt_lib().rt_render_aov(scene, C.byref(f), C.byref(a), 1, None, 1))


def call_aov_through(art, f, scene=FAKE):
    a, t = art.RtAovDesc(), art.RtAovThroughDesc()
    a.albedo, t.max_bounces, t.fuzz_limit = FAKE, 8, 0.0
    return _result(art, art.rt_lib().rt_render_aov_through(scene, C.byref(f), C.byref(a), C.byref(t), 1, None, 1))


HOST_ENTRIES = {"rt_render_adaptive": call_adaptive, "rt_render_variance": call_variance, "rt_render_aov": call_aov,
                "rt_render_aov_through": call_aov_through}


def host_results(art, old_build=False):
    """{entry: {bad frame: (status, detail)}} of the host part (rt_render_adaptive never reads ns: a frame with ns = 0 passes its
    checks, and the fake scene would be dereferenced).  old_build: leave out rt_render_adaptive's tile count, which the build
    before the shared check looked at only after the scene."""
    got = {}
    for entry, call in HOST_ENTRIES.items():
        skip = ["ns = 0"] + (["tile count overflow"] if old_build else []) if entry == "rt_render_adaptive" else []
        got[entry] = {name: call(art, frame(art, **kw)) for name, kw in BAD_FRAMES.items() if name not in skip}
    for entry in ("rt_render_aov", "rt_render_aov_through"):
        got[entry]["46000 x 46000, null scene"] = HOST_ENTRIES[entry](art, frame(art, nx=46000, ny=46000), scene=None)
    return got


def test_host_entries_keep_their_texts(art):
    assert host_results(art) == EXPECT_HOST


# ---- the entries that look at the scene first (one tiny scene on the device; nothing is rendered)
def device_results(art, ds, old_build=False):
    """{entry: {bad frame: (status, detail)}} of the device part.  old_build: leave out the two calls that the build before the
    shared check would have carried out on the 2^28-pixel frame."""
    L = art.rt_lib()
    fb = np.zeros(8 * 8 * 3, np.float32)
    cal, cost, tile_cost, total = np.ones(64, np.uint32), np.zeros(64, np.uint32), np.zeros(1, np.uint32), C.c_uint64(0)
    good = frame(art)
    state = C.c_void_p()
    assert L.rt_progressive_state_create(ds._p, C.byref(good), C.byref(state)) == OK

    def create(f):
        p = C.c_void_p()
        st = _result(art, L.rt_progressive_state_create(ds._p, C.byref(f), C.byref(p)))
        if p:
            L.rt_progressive_state_destroy(ds._p, p)
        return st
    calls = {
        "rt_render": lambda f: _result(art, L.rt_render(ds._p, C.byref(f), fb.ctypes.data, 0, None, 1, None)),
        "rt_render_window": lambda f: _result(art, L.rt_render_window(ds._p, C.byref(f), fb.ctypes.data, 0, state, 0, 2, None, 1, None)),
        "rt_progressive_state_create": create,
        "rt_debug_prior": lambda f: _result(art, L.rt_debug_prior(cal.ctypes.data, 8, 8, f.nx, f.ny, f.tile_rows, f.tile_first, f.tile_stride,
                                                                  cost.ctypes.data, tile_cost.ctypes.data, C.byref(total))),
    }
    got = {}
    try:
        for entry, call in calls.items():
            got[entry] = {}
            for name, kw in BAD_FRAMES.items():
                if name == "ns = 0" and entry in ("rt_render_window", "rt_debug_prior"):
                    continue   # neither reads f->ns: the window would be rendered, the prior takes no sample count
                if old_build and name == "tile count overflow" and entry in ("rt_progressive_state_create", "rt_debug_prior"):
                    continue
                got[entry][name] = call(frame(art, **kw))
    finally:
        L.rt_progressive_state_destroy(ds._p, state)
    return got


@pytest.mark.gpu
def test_device_entries_keep_their_texts(gpu):
    hs = gpu.HostScene("two_spheres", 8, 8)
    ds = gpu.DeviceScene(hs)
    try:
        assert device_results(gpu, ds) == EXPECT_DEVICE
    finally:
        ds.close()
