"""rt_render_variance and rt_denoise_variance without a device: the exports, both descriptors' layouts against the header, the
argument checks that run before any HIP call, the binding's ValueErrors, the CLI's flag rejections -- and properties of the
expectation itself (tests/variance_expect.py), so that the GPU parity tests (tests/test_variance.py,
tests/test_denoise_variance.py) cannot agree with a wrong restatement, and its quality on the oracle's 4-spp frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_expect as ax
import denoise_expect as dx
import variance_expect as vx

RT_ERR_INVALID, RT_ERR_NO_DEVICE = 1, 2
FAKE = 0x10000   # never dereferenced: no check looks at what a pointer points to


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- the library side
def test_variance_symbols_are_exported(art):
    for sym in ("rt_render_variance", "rt_denoise_variance"):
        assert sym in art.RT_ABI_SYMBOLS
        assert hasattr(art.rt_lib(), sym)
    assert art.DENOISE_VARIANCE_DEFAULTS == vx.DEFAULTS


@pytest.mark.parametrize("struct,ctype,size", [("rt_variance_desc", "RtVarianceDesc", 8), ("rt_denoise_variance_desc", "RtDenoiseVarianceDesc", 24)])
def test_desc_layouts_match_header(art, tmp_path, struct, ctype, size):
    """sizeof and every field offset as a C compiler lays out include/rt_abi.h."""
    T = getattr(art, ctype)
    fields = [f for f, _ in T._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   f"  printf(\"%zu\\n\", sizeof({struct}));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof({struct}, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(art.REPO_ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(T) == size
    assert got[1:] == [getattr(T, f).offset for f in fields]


def _frame(art, **kw):
    f = art.RtFrameDesc()
    f.nx, f.ny, f.ns, f.gamma, f.tile_rows, f.tile_first, f.tile_stride = 48, 32, 8, 2.0, 32, 0, 1
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def test_render_variance_argument_checks_name_what_failed(art):
    """Each malformed call is RT_ERR_INVALID with its own text, before any HIP call and before the scene is looked at (the
    scene pointer is a fake one).  A null scene is refused as well, so what passes every check cannot be shown without a device
    scene; tests/test_variance.py covers it."""
    L = art.rt_lib()
    scene = C.c_void_p(FAKE)

    def call(s=scene, f="good", v=4, fb=FAKE, var=FAKE * 64):
        f = _frame(art) if isinstance(f, str) else f
        vd = None if v is None else art.RtVarianceDesc(v, 0)
        st = L.rt_render_variance(s, None if f is None else C.byref(f), None if vd is None else C.byref(vd), fb, 1, var, None, None)
        return st, L.rt_last_error_detail().decode()
    cases = {
        "null scene": dict(s=None), "null frame": dict(f=None), "null desc": dict(v=None), "null fb": dict(fb=None), "null variance_out": dict(var=None),
        "B = 1": dict(v=1), "B = 65": dict(v=65), "B = 0": dict(v=0), "ns % B": dict(v=3), "ns = 0": dict(f=_frame(art, ns=0)),
        "ns < B": dict(f=_frame(art, ns=2)), "nx = 0": dict(f=_frame(art, nx=0)), "2^32 pixels": dict(f=_frame(art, nx=1 << 16, ny=1 << 16, tile_rows=1 << 16)),
        "tile_rows = 0": dict(f=_frame(art, tile_rows=0)), "tile_stride = 0": dict(f=_frame(art, tile_stride=0)),
    }
    texts = {}
    for name, kw in cases.items():
        st, text = call(**kw)
        assert st == RT_ERR_INVALID, (name, st, text)
        assert text.startswith("rt_render_variance: "), (name, text)
        texts[name] = text
    same = [("B = 1", "B = 65", "B = 0"), ("ns % B", "ns = 0", "ns < B"), ("nx = 0", "2^32 pixels"), ("tile_rows = 0", "tile_stride = 0")]
    for group in same:
        assert len({texts[k] for k in group}) == 1, group
    distinct = [g[0] for g in same] + ["null scene", "null frame", "null desc", "null fb", "null variance_out"]
    assert len({texts[k] for k in distinct}) == len(distinct), texts


def _desc(art, **kw):
    d = art.RtDenoiseDesc()
    d.nx, d.ny, d.color, d.out = 48, 32, FAKE, FAKE
    d.iterations, d.normal_sharpness, d.sigma_color, d.color_floor, d.sigma_depth = 5, 4, 0.0, 0.01, 0.2
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _vdesc(art, **kw):
    v = art.RtDenoiseVarianceDesc()
    v.variance, v.sigma_variance, v.variance_floor = FAKE * 6, 3.0, 1e-4
    for k, x in kw.items():
        setattr(v, k, x)
    return v


def _call(art, d, v, on_device=1):
    L = art.rt_lib()
    st = L.rt_denoise_variance(None if d is None else C.byref(d), None if v is None else C.byref(v), on_device, None, 1)
    return st, L.rt_last_error_detail().decode()


def test_denoise_variance_argument_checks_name_what_failed(art):
    """As rt_denoise's (tests/test_denoise_host.py): every malformed description is RT_ERR_INVALID with its own text; one that
    passes every check ends, in a process that has initialised no device, at RT_ERR_NO_DEVICE."""
    inf, nan = float("inf"), float("nan")
    ws = art.denoise_workspace_bytes(48, 32)
    cases = {
        "null d": (None, _vdesc(art)), "null vd": (_desc(art), None),
        "nx = 0": (_desc(art, nx=0), _vdesc(art)), "iterations = 9": (_desc(art, iterations=9), _vdesc(art)),
        "sigma_depth nan": (_desc(art, sigma_depth=nan), _vdesc(art)),
        "sigma_color = 2": (_desc(art, sigma_color=2.0), _vdesc(art)), "sigma_color nan": (_desc(art, sigma_color=nan), _vdesc(art)),
        "sigma_variance = 0": (_desc(art), _vdesc(art, sigma_variance=0.0)), "sigma_variance tiny": (_desc(art), _vdesc(art, sigma_variance=1e-7)),
        "sigma_variance huge": (_desc(art), _vdesc(art, sigma_variance=2e6)), "sigma_variance nan": (_desc(art), _vdesc(art, sigma_variance=nan)),
        "variance_floor = 0": (_desc(art), _vdesc(art, variance_floor=0.0)), "variance_floor < 0": (_desc(art), _vdesc(art, variance_floor=-1.0)),
        "variance_floor inf": (_desc(art), _vdesc(art, variance_floor=inf)),
        "null variance": (_desc(art), _vdesc(art, variance=None)),
        "null color": (_desc(art, color=None), _vdesc(art)),
        "demodulate without albedo": (_desc(art, demodulate=1), _vdesc(art)),
        "small workspace": (_desc(art, workspace=FAKE << 8, workspace_bytes=ws - 1), _vdesc(art)),
        "out overlaps variance": (_desc(art, out=FAKE * 6), _vdesc(art)),
        "variance_out is variance": (_desc(art), _vdesc(art, variance_out=FAKE * 6)),
        "variance_out overlaps color": (_desc(art), _vdesc(art, variance_out=FAKE + 64)),
        "workspace overlaps variance": (_desc(art, workspace=FAKE * 6 - 256, workspace_bytes=ws), _vdesc(art)),
    }
    texts = {}
    for name, (d, v) in cases.items():
        st, text = _call(art, d, v)
        assert st == RT_ERR_INVALID, (name, st, text)
        assert text.startswith("rt_denoise_variance: "), (name, text)
        texts[name] = text
    same = [("sigma_color = 2", "sigma_color nan"), ("sigma_variance = 0", "sigma_variance tiny", "sigma_variance huge", "sigma_variance nan"),
            ("variance_floor = 0", "variance_floor < 0", "variance_floor inf"), ("variance_out is variance", "variance_out overlaps color")]
    for group in same:
        assert len({texts[k] for k in group}) == 1, group
    distinct = [g[0] for g in same] + ["null d", "null vd", "nx = 0", "iterations = 9", "sigma_depth nan", "null variance", "null color",
                                       "demodulate without albedo", "small workspace", "out overlaps variance", "workspace overlaps variance"]
    assert len({texts[k] for k in distinct}) == len(distinct), texts
    good = [(_desc(art), _vdesc(art)), (_desc(art, albedo=FAKE * 2, normal=FAKE * 3, depth=FAKE * 4, demodulate=1), _vdesc(art, variance_out=FAKE * 7)),
            (_desc(art, color_floor=nan, sigma_depth=0.0, normal_sharpness=0, iterations=8), _vdesc(art, sigma_variance=1e-6, variance_floor=1e-30)),
            (_desc(art, workspace=FAKE << 8, workspace_bytes=ws), _vdesc(art))]
    for k, (d, v) in enumerate(good):
        if art._initialised_device is None:
            for on_device in (0, 1):
                st, text = _call(art, d, v, on_device)
                assert st == RT_ERR_NO_DEVICE, (k, on_device, st, text)
        else:
            st, text = _call(art, d, v, 1)
            assert st == RT_ERR_INVALID and "device memory" in text, (k, st, text)
    assert 48 * 32 * 12 < FAKE   # (the fake buffers above do not overlap by accident)


def test_binding_rejects_malformed_input_before_any_device_work(art):
    c = np.zeros((6, 8, 3), np.float32)
    z = np.zeros((6, 8), np.float32)
    bad = [
        lambda: art.denoise(c, variance=c),                                       # shape
        lambda: art.denoise(c, variance=z.astype(np.float64)),                    # dtype
        lambda: art.denoise(c, variance=[[0.0]]),                                 # neither numpy nor torch
        lambda: art.denoise(c, variance=z, variance_out=c),
        lambda: art.denoise(c, variance_out=z),                                   # no variance to filter
        lambda: art.denoise(c, variance=z, sigma_color=2.0),                      # the factors exclude each other
        lambda: art.denoise(c, variance=z, sigma_variance=0.0),
        lambda: art.denoise(c, variance=z, sigma_variance=float("nan")),
        lambda: art.denoise(c, variance=z, sigma_variance=1e7),
        lambda: art.denoise(c, variance=z, variance_floor=0.0),
        lambda: art.denoise(c, variance=z, variance_floor=float("inf")),
        lambda: art.denoise(c, variance=z, iterations=0),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")
    ds = art.DeviceScene.__new__(art.DeviceScene)   # no device scene needed: the checks come first
    ds.device, ds._p = 0, C.c_void_p()
    f = _frame(art)
    rv = [
        lambda: ds.render_variance(f, 1), lambda: ds.render_variance(f, 65), lambda: ds.render_variance(f, 3), lambda: ds.render_variance(f, 2.0),
        lambda: ds.render_variance(f, True), lambda: ds.render_variance(_frame(art, ns=0), 2), lambda: ds.render_variance(_frame(art, nx=0), 2),
        lambda: ds.render_variance(_frame(art, tile_rows=0), 2),
        lambda: ds.render_variance(f, 4, out=np.zeros((32, 48, 3), np.float32)),                                  # one without the other
        lambda: ds.render_variance(f, 4, out=np.zeros((32, 48, 3), np.float32), variance_out=np.zeros((32, 48, 3), np.float32)),
        lambda: ds.render_variance(f, 4, out=np.zeros((32, 48, 3), np.float64), variance_out=np.zeros((32, 48), np.float32)),
        lambda: ds.render_variance(f, 4, out=np.zeros((32, 48, 3), np.float32), variance_out=12345678),            # mixed kinds
        lambda: ds.render_denoised(_frame(art, ns=1), variance=True),                                             # no divisor >= 2
        lambda: ds.render_denoised(_frame(art, ns=17), variance=True),                                            # a prime above 16: none either
        lambda: ds.render_denoised(f, variance=True, batches=3),
        lambda: ds.render_denoised(f, batches=4),                                                                 # batches without variance
        lambda: ds.render_denoised(_frame(art, tile_rows=4, tile_stride=2), variance=True),
    ]
    for k, call in enumerate(rv):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"render case {k} was accepted")


def test_cli_rejects_bad_flag_combinations(art):
    exe = os.path.join(art.LIB_DIR, "rayTracer")
    base = [exe, "--nx", "16", "--ny", "8", "--ns", "4"]
    for extra in (["--denoise-variance"], ["--denoise", "--denoise-variance", "1"], ["--denoise", "--denoise-variance", "65"],
                  ["--denoise", "--denoise-variance", "3"], ["--denoise", "--denoise-variance", "--ns", "1"], ["--denoise", "--denoise-variance", "--ns", "17"],
                  ["--denoise", "--denoise-variance", "--adaptive", "0.1"]):
        r = subprocess.run(base + extra, capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--denoise-variance" in r.stderr and r.stdout == b"", (extra, r.returncode, r.stderr)
    for extra in (["--progressive", "2"], ["--gpus", "2"]):   # what --denoise already rejects
        r = subprocess.run(base + ["--denoise", "--denoise-variance"] + extra, capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--denoise" in r.stderr and r.stdout == b"", (extra, r.returncode, r.stderr)


# -------------------------------------------------------------------------------------- the part-1 expectation (batch means)
def test_equal_batch_means_give_exactly_zero():
    """Frames m_b that are the same triple at every b: T_b = c_b s, y_b = s exactly (c_b s - c_{b-1} s = per s when s is a
    small dyadic number), so Q / B = mu^2 and the variance is exactly 0."""
    m = np.array([[[0.25, 0.5, 0.125], [1.0, 2.0, 4.0]]], np.float32)
    for n, B in [(8, 4), (6, 2), (16, 16), (64, 64)]:
        v = vx.batch_means_variance([m] * B, n, B)
        assert v.dtype == np.float32 and v.shape == (1, 2) and (_bits(v) == 0).all(), (n, B, v)
    nan = np.full((1, 1, 3), np.nan, np.float32)
    assert (_bits(vx.batch_means_variance([nan] * 4, 8, 4)) == 0).all()          # a NaN gives 0


def test_b_equal_n_is_the_sample_variance_of_the_mean(orc):
    """B = n on an oracle frame: y_b is then sample b's own r + g + b (recovered from consecutive frames), and the result is
    np.var(y, ddof=1) / n to 1e-6 relative.  The contract's one-pass form Q / B - mu^2 cancels: in double its error is a few
    2^-53 of mean(y^2), so the relative bound is asked where var(y) >= 1e-8 mean(y^2) (error <= ~1e-7 of the variance) and
    an absolute one, 1e-13 mean(y^2) / n, elsewhere (pixels that see one constant colour)."""
    n = 16
    ex = ax.Expectation(orc.OracleScene("cornell", 32, 24))
    frames = [ex.frame(b) for b in range(1, n + 1)]
    got = vx.batch_means_variance(frames, n, n).astype(np.float64)
    T = np.stack([np.float64(b) * ((f[..., 0].astype(np.float64) + f[..., 1]) + f[..., 2]) for b, f in zip(range(1, n + 1), frames)])
    y = np.diff(np.concatenate([np.zeros((1,) + T.shape[1:]), T]), axis=0)
    want = np.var(y, axis=0, ddof=1) / n
    second = (y ** 2).mean(axis=0)
    noisy = np.var(y, axis=0) >= 1e-8 * second
    assert noisy.mean() > 0.5, noisy.mean()
    # (got is the float32 the contract stores: 2^-24 relative on top)
    assert np.allclose(got[noisy], want[noisy], rtol=1e-6, atol=0), float(np.max(np.abs(got[noisy] / want[noisy] - 1)))
    assert (np.abs(got[~noisy] - want[~noisy]) <= 1e-13 * second[~noisy] / n + 1e-30).all()


# ------------------------------------------------------------------------------- the part-2 expectation (the filter itself)
OFF = dict(normal_sharpness=0, sigma_depth=0.0)


@pytest.mark.parametrize("nx,ny", [(3, 2), (21, 13)])
def test_constant_image_and_variance(nx, ny):
    """A constant image with a constant variance c, every guide off: d1 = 0, so every factor is 1 and the weights are
    rt_denoise's exact ones -- the image comes back bit for bit.  variance_out(p) = sum(w^2 v_q) / (sum w)^2 is at most
    max(v) sum(w^2) / (sum w)^2, so it is at most c everywhere and its maximum never grows with K; the maximum shrinks with every
    iteration in which each pixel has a tap beside the centre inside the image (2 s - 1 < nx or ny).  It does not shrink pixel
    by pixel near a border: a pixel there may take taps whose variance is larger than its own."""
    img = np.full((ny, nx, 3), 0.5, np.float32)
    c = np.float32(0.375)
    var = np.full((ny, nx), c, np.float32)
    last = c
    for K in range(1, 6):
        out, vout = vx.denoise_variance(img, var, iterations=K, sigma_variance=3.0, variance_floor=1e-4, **OFF)
        assert out.dtype == vout.dtype == np.float32 and np.array_equal(_bits(out), _bits(img)), K
        assert (vout <= c).all() and (vout > 0).all(), K
        s = 1 << (K - 1)
        assert vout.max() <= last, K
        if 2 * s - 1 < max(nx, ny):
            assert vout.max() < last, K
        last = vout.max()


def _step(nx=24, ny=16, lo=0.25, hi=1.0):
    img = np.empty((ny, nx, 3), np.float32)
    img[:, :nx // 2], img[:, nx // 2:] = lo, hi
    return img


def test_a_step_above_the_noise_holds_and_one_below_the_floor_smears():
    """Step 0.25 | 1.0: d1 = 2.25 across it.  With variance 0.01 and sigma = 3, sigma sqrt(vp + vq) = 0.42 < 2.25: r > 1, the
    factor is 0 and nothing crosses -- each half comes back bit for bit.  With a floor of 100 the same step is below it
    (r = 5.06 / 100.2): taps cross and the edge smears."""
    img = _step()
    var = np.full(img.shape[:2], 0.01, np.float32)
    for K in (1, 3, 5):
        out, _ = vx.denoise_variance(img, var, iterations=K, sigma_variance=3.0, variance_floor=1e-4, **OFF)
        assert np.array_equal(_bits(out), _bits(img)), K
        smeared, _ = vx.denoise_variance(img, var, iterations=K, sigma_variance=3.0, variance_floor=100.0, **OFF)
        assert not np.array_equal(smeared, img) and 0.25 < smeared[8, 11, 0] < 1.0, K


def test_variance_widens_what_crosses():
    """The same small step crosses where the variance says it is noise and not where it says the pixels are clean."""
    img = _step(lo=0.5, hi=0.625)      # d1 = 0.375
    kw = dict(iterations=2, sigma_variance=3.0, variance_floor=1e-6, **OFF)
    clean, _ = vx.denoise_variance(img, np.full(img.shape[:2], 1e-4, np.float32), **kw)      # 3 sqrt(2e-4) = 0.04 < 0.375
    noisy, _ = vx.denoise_variance(img, np.full(img.shape[:2], 0.01, np.float32), **kw)      # 3 sqrt(0.02) = 0.42 > 0.375
    assert np.array_equal(_bits(clean), _bits(img))
    assert 0.5 < noisy[8, 11, 0] < 0.625


def test_preblur_and_demodulation_of_the_variance():
    """One bright variance pixel spreads 3x3 with weights 1/4, 1/8, 1/16; with demodulation by a grey albedo a = 1/2 the
    variance is carried by t^2 = 4 going in and 1/4 coming out."""
    u = np.zeros((5, 7), np.float32)
    u[2, 3] = 16.0
    v0 = vx.preblur(u)
    assert v0[2, 3] == 4.0 and v0[2, 2] == 2.0 and v0[1, 2] == 1.0 and v0[0, 3] == 0.0
    assert vx.preblur(np.full((1, 1), 3.0, np.float32))[0, 0] == 3.0 and vx.preblur(np.full((2, 3), 3.0, np.float32)).tolist() == [[3.0] * 3] * 2
    img = np.full((5, 7, 3), 0.25, np.float32)
    alb = np.full((5, 7, 3), 0.5, np.float32)
    var = np.full((5, 7), 0.375, np.float32)
    out_d, v_d = vx.denoise_variance(img, var, alb, iterations=2, sigma_variance=3.0, variance_floor=1e-4, **OFF)
    out_p, v_p = vx.denoise_variance(img, var, iterations=2, sigma_variance=3.0, variance_floor=1e-4, **OFF)
    assert np.array_equal(_bits(out_d), _bits(img)) and np.array_equal(_bits(v_d), _bits(v_p))


def test_synthetic_inputs_exercise_every_factor():
    """The GPU test's inputs: finite results, a variance that is 0 in places, and each factor changes the result."""
    s = dx.synthetic(65, 33, 1)
    var = vx.synthetic_variance(65, 33, 1)
    assert (var >= 0).all() and (var == 0).any() and (var > 0).any()
    kw = dict(iterations=5, normal_sharpness=4, sigma_depth=0.2, **vx.DEFAULTS)
    full, vfull = vx.denoise_variance(s["color"], var, s["albedo"], s["normal"], s["depth"], **kw)
    assert np.isfinite(full).all() and np.isfinite(vfull).all() and (vfull >= 0).all() and full.dtype == vfull.dtype == np.float32
    for off in (dict(normal_sharpness=0), dict(sigma_depth=0.0), dict(sigma_variance=1e6), dict(demodulate=False)):
        other, vother = vx.denoise_variance(s["color"], var, s["albedo"], s["normal"], s["depth"], **dict(kw, **off))
        assert np.isfinite(other).all() and not np.array_equal(other, full) and not np.array_equal(vother, vfull), off
    plain = dx.denoise(s["color"], s["albedo"], s["normal"], s["depth"], **dx.DEFAULTS)
    assert not np.array_equal(plain, full)


# ------------------------------------------------------------------------------------------------------------- quality
QUALITY_NX, QUALITY_NY = 96, 64
# RMSE(filtered) / RMSE(noisy) from tools/variance_sweep.py: (colour factor, variance-guided at the defaults)
MEASURED = {"spheres_plain/1": (0.954, 0.952), "spheres_tex/3": (0.964, 0.958), "general_plain/1": (0.706, 0.712),
            "general_tex/4": (0.838, 0.806), "bouncing": (0.930, 0.941), "final": (0.946, 0.923)}
BEATS_COLOUR_FACTOR = ["spheres_plain/1", "spheres_tex/3", "general_tex/4", "final"]


@pytest.mark.parametrize("key", ["spheres_plain/1", "general_plain/1", "spheres_tex/3", "general_tex/4", "final"])
def test_variance_guided_frame_is_closer_to_the_truth(art, orc, key):
    """The oracle's 4-spp frame with the oracle-side feature buffers and the batch-means variance at B = 4, filtered with the
    binding's defaults, against the oracle at 256 spp and another seed.  RMSE(variance-guided) < RMSE(noisy) on every frame
    here; RMSE(variance-guided) < RMSE(colour-factor denoiser) on the frames where the sweep shows it (MEASURED: 0.952 < 0.954,
    0.958 < 0.964, 0.806 < 0.838, 0.923 < 0.946) and not asserted on general_plain/1 (0.712 > 0.706) or bouncing (0.941 > 0.930)."""
    f = vx.oracle_frame(art, orc, key, ns=4, batches=4, nx=QUALITY_NX, ny=QUALITY_NY)
    truth, _ = f["oracle"].render(256, gamma=1.0, seed_base=77_000_000_019)
    shared = {k: art.DENOISE_DEFAULTS[k] for k in ("iterations", "normal_sharpness", "sigma_depth")}
    out, _ = vx.denoise_variance(f["color"], f["variance"], f["albedo"], f["normal"], f["depth"], **shared, **art.DENOISE_VARIANCE_DEFAULTS)
    col = dx.denoise(f["color"], f["albedo"], f["normal"], f["depth"], **art.DENOISE_DEFAULTS)

    def rmse(a):
        return float(np.sqrt(np.mean((a.astype(np.float64) - truth) ** 2)))
    noisy = rmse(f["color"])
    print(f"{key}: RMSE noisy {noisy:.5f}, colour factor {rmse(col) / noisy:.4f}, variance-guided {rmse(out) / noisy:.4f}")
    assert rmse(out) < noisy
    if key in BEATS_COLOUR_FACTOR:
        assert rmse(out) < rmse(col)
