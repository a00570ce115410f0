"""rt_denoise without a device: the exports, the descriptor's layout against the header, the workspace size, the argument
checks that run before any HIP call, the option, the binding's ValueErrors, the CLI's flag rejections -- and properties of the
expectation itself (tests/denoise_expect.py), so that the GPU parity test (tests/test_denoise.py) cannot agree with a wrong
restatement, and its quality on the oracle's 4-spp frames with the binding's defaults."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_expect as dx

RT_ERR_INVALID, RT_ERR_NO_DEVICE = 1, 2
FAKE = 0x10000   # never dereferenced: no check looks at what a pointer points to


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- the library side
def test_denoise_is_exported(art):
    for sym in ("rt_denoise", "rt_denoise_workspace_bytes"):
        assert sym in art.RT_ABI_SYMBOLS
        assert hasattr(art.rt_lib(), sym)


def test_denoise_desc_layout_matches_header(art, tmp_path):
    """sizeof and every field offset of rt_denoise_desc as a C compiler lays out include/rt_abi.h."""
    fields = [f for f, _ in art.RtDenoiseDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(rt_denoise_desc));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof(rt_denoise_desc, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(art.REPO_ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(art.RtDenoiseDesc) == 96
    assert got[1:] == [getattr(art.RtDenoiseDesc, f).offset for f in fields]


def test_workspace_bytes(art):
    """Three images of 16-byte records (two colour images and the guides), each rounded up to 256 bytes; 0 for a bad size."""
    for nx, ny in [(1, 1), (5, 3), (65, 33), (1200, 800), (1 << 15, (1 << 16) - 1)]:
        want = 3 * ((nx * ny * 16 + 255) // 256 * 256)
        assert art.denoise_workspace_bytes(nx, ny) == want, (nx, ny)
    for nx, ny in [(0, 4), (4, 0), (-1, 4), (4, -7), (1 << 16, 1 << 15), (1 << 16, 1 << 16)]:
        assert art.denoise_workspace_bytes(nx, ny) == 0, (nx, ny)


def _desc(art, **kw):
    d = art.RtDenoiseDesc()
    d.nx, d.ny, d.color, d.out = 48, 32, FAKE, FAKE
    d.iterations, d.normal_sharpness, d.sigma_color, d.color_floor, d.sigma_depth = 5, 4, 2.0, 0.01, 0.2
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(art, d, on_device=1):
    L = art.rt_lib()
    st = L.rt_denoise(None if d is None else C.byref(d), on_device, None, 1)
    return st, L.rt_last_error_detail().decode()


def test_argument_checks_name_what_failed(art):
    """Each malformed description is RT_ERR_INVALID with its own text.  A description that passes every check ends, in a process
    that has initialised no device, at RT_ERR_NO_DEVICE: the checks come before any HIP call.  (In a process that has one,
    its fake pointers are then refused as not being device memory.)"""
    inf, nan = float("inf"), float("nan")
    px = 48 * 32
    cases = {
        "null d": None,
        "nx = 0": _desc(art, nx=0),
        "ny < 0": _desc(art, ny=-3),
        "2^32 pixels": _desc(art, nx=1 << 16, ny=1 << 16),
        "iterations = 0": _desc(art, iterations=0),
        "iterations = 9": _desc(art, iterations=9),
        "normal_sharpness = -1": _desc(art, normal_sharpness=-1),
        "normal_sharpness = 11": _desc(art, normal_sharpness=11),
        "sigma_depth < 0": _desc(art, sigma_depth=-0.1),
        "sigma_depth tiny": _desc(art, sigma_depth=1e-7),
        "sigma_depth nan": _desc(art, sigma_depth=nan),
        "sigma_color huge": _desc(art, sigma_color=2e6),
        "sigma_color inf": _desc(art, sigma_color=inf),
        "color_floor = 0": _desc(art, color_floor=0.0),
        "color_floor nan": _desc(art, color_floor=nan),
        "null color": _desc(art, color=None),
        "null out": _desc(art, out=None),
        "demodulate without albedo": _desc(art, demodulate=1),
        "small workspace": _desc(art, workspace=FAKE << 8, workspace_bytes=art.denoise_workspace_bytes(48, 32) - 1),
        "out overlaps color": _desc(art, out=FAKE + 12),
        "out is albedo": _desc(art, albedo=FAKE << 4, out=FAKE << 4),
        "workspace overlaps depth": _desc(art, depth=(FAKE << 8) + 64, workspace=FAKE << 8, workspace_bytes=art.denoise_workspace_bytes(48, 32)),
    }
    texts = {}
    for name, d in cases.items():
        st, text = _call(art, d)
        assert st == RT_ERR_INVALID, (name, st, text)
        assert text.startswith("rt_denoise"), (name, text)
        texts[name] = text
    same = [("nx = 0", "ny < 0"), ("iterations = 0", "iterations = 9"), ("normal_sharpness = -1", "normal_sharpness = 11"),
            ("sigma_depth < 0", "sigma_depth tiny", "sigma_depth nan"), ("sigma_color huge", "sigma_color inf"),
            ("color_floor = 0", "color_floor nan"), ("out overlaps color", "out is albedo")]
    for group in same:
        assert len({texts[k] for k in group}) == 1, group
    distinct = [g[0] for g in same] + ["null d", "2^32 pixels", "null color", "null out", "demodulate without albedo", "small workspace",
                                       "workspace overlaps depth"]
    assert len({texts[k] for k in distinct}) == len(distinct), texts
    # what passes: the plain description, in place, every guide, a zero sigma with any floor, a large enough workspace
    good = [_desc(art), _desc(art, albedo=FAKE * 2, normal=FAKE * 3, depth=FAKE * 4, demodulate=1), _desc(art, sigma_color=0.0, color_floor=nan),
            _desc(art, sigma_depth=0.0, normal_sharpness=0, iterations=8), _desc(art, out=FAKE * 5),
            _desc(art, workspace=FAKE << 8, workspace_bytes=art.denoise_workspace_bytes(48, 32))]
    for k, d in enumerate(good):
        if art._initialised_device is None:
            for on_device in (0, 1):
                st, text = _call(art, d, on_device)
                assert st == RT_ERR_NO_DEVICE, (k, on_device, st, text)
        else:
            st, text = _call(art, d, 1)
            assert st == RT_ERR_INVALID and "device memory" in text, (k, st, text)
    assert px * 12 < FAKE   # (the fake buffers above do not overlap by accident)


def test_denoise_option(art):
    L = art.rt_lib()
    try:
        for v in (-1, 0, 1):
            assert L.rt_set_option(b"denoise_lds", v) == 0, v
        for v in (-2, 2):
            assert L.rt_set_option(b"denoise_lds", v) == RT_ERR_INVALID, v
            assert "denoise_lds" in L.rt_last_error_detail().decode()
    finally:
        assert L.rt_reset_options() == 0


def test_binding_defaults_are_the_expectation_s(art):
    assert art.DENOISE_DEFAULTS == dx.DEFAULTS


def test_binding_rejects_malformed_input_before_any_device_work(art):
    c = np.zeros((6, 8, 3), np.float32)
    z = np.zeros((6, 8), np.float32)
    ok = dict(dx.DEFAULTS)
    bad = [
        lambda: art.denoise([[0.0] * 3], **ok),                                   # neither numpy nor torch
        lambda: art.denoise(z, **ok),                                             # not (ny, nx, 3)
        lambda: art.denoise(np.zeros((0, 8, 3), np.float32), **ok),
        lambda: art.denoise(c.astype(np.float64), **ok),                          # dtype
        lambda: art.denoise(np.zeros((6, 8, 6), np.float32)[:, :, ::2], **ok),    # not contiguous
        lambda: art.denoise(c, albedo=z, **ok),                                   # shape of a guide
        lambda: art.denoise(c, depth=c, **ok),
        lambda: art.denoise(c, normal=c.astype(np.float64), **ok),
        lambda: art.denoise(c, out=np.zeros((6, 8), np.float32), **ok),
        lambda: art.denoise(c, demodulate=True, **ok),                            # no albedo to divide by
        lambda: art.denoise(c, workspace=np.zeros(1 << 16, np.uint8), **ok),      # a host workspace
        lambda: art.denoise(c, **dict(ok, iterations=0)),
        lambda: art.denoise(c, **dict(ok, iterations=9)),
        lambda: art.denoise(c, **dict(ok, iterations=2.0)),
        lambda: art.denoise(c, **dict(ok, normal_sharpness=11)),
        lambda: art.denoise(c, **dict(ok, sigma_color=-1.0)),
        lambda: art.denoise(c, **dict(ok, sigma_color=float("nan"))),
        lambda: art.denoise(c, **dict(ok, sigma_depth=1e7)),
        lambda: art.denoise(c, **dict(ok, color_floor=0.0)),
        lambda: art.denoise(c, **dict(ok, color_floor=float("inf"))),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")
    ds = art.DeviceScene.__new__(art.DeviceScene)   # no device scene needed: the check comes first
    ds.device, ds._p = 0, C.c_void_p()
    f = art.RtFrameDesc()
    f.nx, f.ny, f.ns, f.gamma, f.tile_rows, f.tile_first, f.tile_stride = 48, 32, 4, 2.0, 4, 0, 2
    with pytest.raises(ValueError):
        ds.render_denoised(f)
    f.tile_rows, f.tile_stride, f.tile_first = 32, 1, 1
    with pytest.raises(ValueError):
        ds.render_denoised(f)


def test_cli_rejects_denoise_with_progressive_and_several_gpus(art):
    exe = os.path.join(art.LIB_DIR, "rayTracer")
    for extra in (["--progressive", "2"], ["--gpus", "2"], ["--denoise", "9"], ["--denoise", "0"]):
        r = subprocess.run([exe, "--nx", "16", "--ny", "8", "--ns", "2", "--denoise"] + extra, capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--denoise" in r.stderr and r.stdout == b"", (extra, r.returncode, r.stderr)


# ------------------------------------------------------------------------------------------------- the expectation itself
OFF = dict(sigma_color=0.0, color_floor=0.01, normal_sharpness=0, sigma_depth=0.0)


@pytest.mark.parametrize("nx,ny", [(3, 2), (21, 13)])
def test_constant_image_returns_bit_for_bit(nx, ny):
    """(a) All guides off: every weight is a product of powers of two and threes, W and S = 0.5 W are exact whichever taps
    are skipped, so 0.5 comes back -- also at 3 x 2, where most taps are outside the image."""
    c = np.full((ny, nx, 3), 0.5, np.float32)
    for K in range(1, 6):
        out = dx.denoise(c, iterations=K, **OFF)
        assert out.dtype == np.float32 and np.array_equal(_bits(out), _bits(c)), K


def _half_planes(nx=24, ny=16):
    c = np.empty((ny, nx, 3), np.float32)
    c[:, :nx // 2], c[:, nx // 2:] = 0.25, 1.0
    n = np.zeros((ny, nx, 3), np.float32)
    n[:, :nx // 2, 0], n[:, nx // 2:, 2] = 1.0, 1.0
    z = np.empty((ny, nx), np.float32)
    z[:, :nx // 2], z[:, nx // 2:] = 1.0, 2.0
    return c, n, z


@pytest.mark.parametrize("K", [1, 3, 5])
def test_nothing_crosses_a_normal_edge(K):
    """(b) Orthogonal normals, normal_sharpness = 1: taps across the edge weigh exactly 0, taps on a pixel's own side exactly
    H H, so each half is (a) for its own constant."""
    c, n, _ = _half_planes()
    out = dx.denoise(c, normal=n, iterations=K, **dict(OFF, normal_sharpness=1))
    assert np.array_equal(_bits(out), _bits(c))
    blurred = dx.denoise(c, iterations=K, **OFF)
    assert not np.array_equal(blurred, c)          # without the guide the edge does smear: the guide is what held it


@pytest.mark.parametrize("K", [1, 3, 5])
def test_nothing_crosses_a_depth_edge(K):
    """(c) Depth 1 against 2 at sigma_depth = 0.1: r = 1 / (0.1 * 2 + 1e-20) = 5, t = max(1 - 5, 0) = 0; same depth: r = 0."""
    c, n, z = _half_planes()
    out = dx.denoise(c, normal=n, depth=z, iterations=K, **dict(OFF, sigma_depth=0.1))   # (normal_sharpness = 0: normals off)
    assert np.array_equal(_bits(out), _bits(c))


def test_colour_factor_holds_an_edge_and_lets_equal_colours_through():
    """The colour factor alone: 0.25 against 1.0 at sigma_color = 0.5 gives r = 2.25 / (0.5 * (3.75 + 2^-7)) > 1 -> 0."""
    c, _, _ = _half_planes()
    out = dx.denoise(c, iterations=3, **dict(OFF, sigma_color=0.5, color_floor=2.0 ** -7))
    assert np.array_equal(_bits(out), _bits(c))


def test_demodulation_is_exact_on_exact_inputs():
    """(d) color = albedo * 0.5 with albedo a multiple of 2^-8 in [2^-4, 1]: the quotient is 0.5 everywhere, the filter
    returns 0.5 ((a), whatever the colour factor does with equal colours) and the product albedo * 0.5 is exact."""
    rng = np.random.default_rng(5)
    albedo = (rng.integers(16, 257, (13, 21, 3)) / 256.0).astype(np.float32)
    color = (albedo * np.float32(0.5)).astype(np.float32)
    out = dx.denoise(color, albedo, iterations=4, **dict(OFF, sigma_color=1.0))
    assert np.array_equal(_bits(out), _bits(color))
    assert not np.array_equal(dx.denoise(color, albedo, iterations=4, demodulate=False, **OFF), color)


def test_synthetic_inputs_exercise_every_factor():
    """The GPU test's inputs: finite results, and each factor changes the result (so that none is tested as a no-op)."""
    s = dx.synthetic(65, 33, 1)
    assert (s["color"] > 0).all() and (s["albedo"] < 2.0 ** -10).any() and (s["depth"] == 0).any() and (s["depth"] > 0).any()
    lens = np.linalg.norm(s["normal"], axis=2)
    assert (np.abs(lens - 1) < 1e-6).any() and ((lens > 0.05) & (lens < 0.9)).any() and (lens == 0).any()
    full = dx.denoise(**s, **dx.DEFAULTS)
    assert np.isfinite(full).all() and full.dtype == np.float32
    for off in (dict(normal_sharpness=0), dict(sigma_depth=0.0), dict(sigma_color=0.0)):
        other = dx.denoise(**s, **dict(dx.DEFAULTS, **off))
        assert np.isfinite(other).all() and not np.array_equal(other, full), off


# ------------------------------------------------------------------------------------------------------------- quality
QUALITY_NX, QUALITY_NY = 96, 64


@pytest.mark.parametrize("key", ["spheres_plain/1", "general_plain/1"])
def test_denoised_frame_is_closer_to_the_truth_than_the_noisy_one(art, orc, key):
    """The oracle's 4-spp frame of a scene_gen scene with the oracle-side feature buffers, filtered with the binding's
    defaults, against the oracle at 256 spp and another seed: RMSE(denoised, truth) < RMSE(noisy, truth).  Measured ratios:
    DESIGN.md 4.11 (0.95 and 0.71 on these two)."""
    f = dx.oracle_frame(art, orc, key, ns=4, nx=QUALITY_NX, ny=QUALITY_NY)
    truth, _ = f["oracle"].render(256, gamma=1.0, seed_base=77_000_000_019)
    out = dx.denoise(f["color"], f["albedo"], f["normal"], f["depth"], **art.DENOISE_DEFAULTS)

    def rmse(a):
        return float(np.sqrt(np.mean((a.astype(np.float64) - truth) ** 2)))
    print(f"{key}: RMSE noisy {rmse(f['color']):.4f}, denoised {rmse(out):.4f}, ratio {rmse(out) / rmse(f['color']):.3f}")
    assert rmse(out) < rmse(f["color"])
