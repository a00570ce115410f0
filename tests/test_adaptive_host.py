"""rt_render_adaptive without a device: the export, the descriptor's layout against the header, the argument checks that run
before any HIP call, and the invariants of the expectation helper the GPU tests compare against."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_expect as ax

RT_ERR_INVALID = 1
FAKE = 0x1000   # never dereferenced: every check below fails before a pointer is looked at


def test_render_adaptive_is_exported(art):
    assert "rt_render_adaptive" in art.RT_ABI_SYMBOLS
    assert hasattr(art.rt_lib(), "rt_render_adaptive")


def test_adaptive_desc_layout_matches_header(art, tmp_path):
    """sizeof and every field offset of rt_adaptive_desc as a C compiler lays out include/rt_abi.h."""
    fields = [f for f, _ in art.RtAdaptiveDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(rt_adaptive_desc));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof(rt_adaptive_desc, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(art.REPO_ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(art.RtAdaptiveDesc) == 16
    assert got[1:] == [getattr(art.RtAdaptiveDesc, f).offset for f in fields]


def _frame(art, **kw):
    f = art.RtFrameDesc()
    f.nx, f.ny, f.ns, f.gamma = 8, 8, 1, 1.0
    f.tile_rows, f.tile_first, f.tile_stride = 8, 0, 1
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _desc(art, min_spp=4, max_spp=16, threshold=0.1, floor=0.01):
    return art.RtAdaptiveDesc(min_spp, max_spp, threshold, floor)


def _call(art, scene, f, a, fb=FAKE):
    L = art.rt_lib()
    st = L.rt_render_adaptive(scene, None if f is None else C.byref(f), None if a is None else C.byref(a), fb, 1, None, None, None)
    return st, L.rt_last_error_detail().decode()


def test_argument_checks_name_what_failed(art):
    """A fake (never dereferenced) scene pointer: each check must fire before the scene or any HIP call is touched."""
    inf, nan = float("inf"), float("nan")
    cases = {
        "null scene": (None, _frame(art), _desc(art), FAKE, "null scene"),
        "null frame": (FAKE, None, _desc(art), FAKE, "null frame"),
        "null adaptive desc": (FAKE, _frame(art), None, FAKE, "null adaptive"),
        "null fb": (FAKE, _frame(art), _desc(art), None, "null fb"),
        "odd min_spp": (FAKE, _frame(art), _desc(art, 3, 12), FAKE, "min_spp"),
        "min_spp 0": (FAKE, _frame(art), _desc(art, 0, 0), FAKE, "min_spp"),
        "negative min_spp": (FAKE, _frame(art), _desc(art, -2, 4), FAKE, "min_spp"),
        "max below min": (FAKE, _frame(art), _desc(art, 8, 4), FAKE, "max_spp"),
        "max not a power-of-two multiple": (FAKE, _frame(art), _desc(art, 4, 24), FAKE, "max_spp"),
        "K = 17": (FAKE, _frame(art), _desc(art, 2, 2 << 17), FAKE, "max_spp"),
        "NaN threshold": (FAKE, _frame(art), _desc(art, threshold=nan), FAKE, "threshold"),
        "infinite threshold": (FAKE, _frame(art), _desc(art, threshold=-inf), FAKE, "threshold"),
        "negative floor": (FAKE, _frame(art), _desc(art, floor=-0.5), FAKE, "floor"),
        "NaN floor": (FAKE, _frame(art), _desc(art, floor=nan), FAKE, "floor"),
        "infinite floor": (FAKE, _frame(art), _desc(art, floor=inf), FAKE, "floor"),
        "zero width": (FAKE, _frame(art, nx=0), _desc(art), FAKE, "frame size"),
        "negative height": (FAKE, _frame(art, ny=-4), _desc(art), FAKE, "frame size"),
        "frame too large": (FAKE, _frame(art, nx=1 << 16, ny=1 << 15), _desc(art), FAKE, "frame size"),
        "zero tile rows": (FAKE, _frame(art, tile_rows=0), _desc(art), FAKE, "partition"),
        "zero tile stride": (FAKE, _frame(art, tile_stride=0), _desc(art), FAKE, "partition"),
        "negative first tile": (FAKE, _frame(art, tile_first=-1), _desc(art), FAKE, "partition"),
    }
    for name, (scene, f, a, fb, word) in cases.items():
        st, detail = _call(art, scene, f, a, fb)
        assert st == RT_ERR_INVALID, (name, st, detail)
        assert detail.startswith("rt_render_adaptive:") and word in detail, (name, detail)


def test_largest_k_is_accepted_by_the_checks(art):
    """K = 16 and K = 0 pass every argument check: with a null scene the scene check is what fails."""
    for a in (_desc(art, 2, 2 << 16), _desc(art, 6, 6), _desc(art, threshold=-1.0, floor=0.0)):
        st, detail = _call(art, None, _frame(art), a)
        assert st == RT_ERR_INVALID and "null scene" in detail


def test_python_raises_value_error_before_launch(art):
    """DeviceScene.render_adaptive's own checks; the object is never initialised on a device."""
    ds = art.DeviceScene.__new__(art.DeviceScene)
    ds._p, ds.device = C.c_void_p(), 0
    f = _frame(art)
    bad = [dict(min_spp=3, max_spp=12), dict(min_spp=4, max_spp=12), dict(min_spp=4, max_spp=2), dict(min_spp=2, max_spp=2 << 17),
           dict(min_spp=4, max_spp=16, threshold=float("nan")), dict(min_spp=4, max_spp=16, floor=-1.0),
           dict(min_spp=4, max_spp=16, threshold=1e39), dict(min_spp=4.0, max_spp=16)]
    for kw in bad:
        kw.setdefault("threshold", 0.1)
        with pytest.raises(ValueError):
            ds.render_adaptive(f, **kw)
    with pytest.raises(ValueError):
        ds.render_adaptive(_frame(art, tile_rows=0), 4, 16, 0.1)


# ---- the expectation helper on synthetic averages (no oracle render needed)

def _linear(rng, n_levels, shape=(6, 7)):
    return [rng.random(shape + (3,), dtype=np.float32) for _ in range(n_levels)]


def _frames(levels, min_spp):
    ns = [min_spp // 2] + [min_spp << k for k in range(len(levels) - 1)]
    return dict(zip(ns, levels))


def test_negative_threshold_keeps_every_pixel_to_max():
    rng = np.random.default_rng(1)
    lin = _frames(_linear(rng, 5), 4)
    lin[4] = lin[2].copy()   # identical averages: d = 0 would pass any non-negative threshold
    spp = ax.spp_map(lin, 4, 32, -1.0, 0.0)
    assert (spp == 32).all()
    assert (ax.spp_map(lin, 4, 32, 0.0, 0.0)[...] == 4).all()


def test_k0_gives_min_spp_everywhere():
    rng = np.random.default_rng(2)
    lin = _frames(_linear(rng, 2), 8)
    for t in (-1.0, 0.0, 0.5, 100.0):
        assert (ax.spp_map(lin, 8, 8, t, 0.01) == 8).all()


def test_larger_threshold_never_raises_a_count():
    rng = np.random.default_rng(3)
    lin = _frames(_linear(rng, 6), 2)
    prev = None
    for t in (0.0, 0.05, 0.1, 0.3, 0.7, 1.5, 4.0):
        spp = ax.spp_map(lin, 2, 32, t, 0.02)
        if prev is not None:
            assert (spp <= prev).all(), t
        prev = spp
    assert len(np.unique(ax.spp_map(lin, 2, 32, 0.7, 0.02))) >= 2


def test_hand_worked_pixel():
    """One pixel by hand: h at 2 = (0.5, 0.25, 0.125), a at 4 = (0.5, 0.375, 0.125): d = 0.125, s = 1.0.
    With floor 0.25 it converges at 4 iff threshold >= 0.1 (0.1 * 1.25 = 0.125); at 8 the average is unchanged."""
    h = np.array([[[0.5, 0.25, 0.125]]], np.float32)
    a = np.array([[[0.5, 0.375, 0.125]]], np.float32)
    lin = {2: h, 4: a, 8: a.copy(), 16: a.copy()}
    assert ax.spp_map(lin, 4, 16, 0.1, 0.25)[0, 0] == 4
    assert ax.spp_map(lin, 4, 16, 0.09, 0.25)[0, 0] == 8        # not at 4; at 8, d = 0
    assert ax.spp_map(lin, 4, 16, -0.1, 0.25)[0, 0] == 16
    d, s = 0.125, 1.0
    assert d <= np.float64(np.float32(0.1)) * (s + 0.25) and not d <= np.float64(np.float32(0.09)) * (s + 0.25)


def test_nan_never_converges():
    h = np.array([[[0.5, np.nan, 0.1]]], np.float32)
    a = np.array([[[0.5, 0.5, 0.1]]], np.float32)
    lin = {2: h, 4: a, 8: np.full_like(a, np.nan), 16: a}
    assert ax.spp_map(lin, 4, 16, 1e30, 1.0)[0, 0] == 16


def test_helper_on_an_oracle_frame(orc):
    """The helper end to end on a tiny oracle frame: counts come from the checkpoints, and the ray total at K = 0 is the
    oracle's own count at min_spp."""
    o = orc.OracleScene("bouncing", 12, 8)
    e = ax.Expectation(o)
    fb, spp, rays, samples = e.predict(2, 8, 0.2, 0.01)
    assert set(np.unique(spp)) <= {2, 4, 8}
    _, cnt = o.render(2)
    fb0, spp0, rays0, _ = e.predict(2, 2, 0.2, 0.01)
    assert (spp0 == 2).all() and int(rays0.sum()) == cnt["rays"]
    assert np.array_equal(fb0.view(np.uint32), e.frame(2).view(np.uint32))
