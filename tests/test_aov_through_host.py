"""rt_render_aov_through without a device: the export, the descriptor's layout against the header, the argument checks that run
before any HIP call, the option, the binding's ValueErrors, the NumPy restatement of the chain's arithmetic against optics in
float64 -- and the conditions on the expectation's side that keep the GPU test (tests/test_aov_through.py) from testing nothing,
checked on the very scenes, frames and parameters it uses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aov_expect as ax
import aov_through_expect as tx
import scene_gen as sg

RT_ERR_INVALID = 1
FAKE = 0x1000   # never dereferenced: every check below fails before a pointer is looked at
F = np.float32


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- the library side
def test_render_aov_through_is_exported(art):
    assert "rt_render_aov_through" in art.RT_ABI_SYMBOLS
    assert hasattr(art.rt_lib(), "rt_render_aov_through")


def test_through_desc_layout_matches_header(art, tmp_path):
    """sizeof and every field offset of rt_aov_through_desc as a C compiler lays out include/rt_abi.h."""
    fields = [f for f, _ in art.RtAovThroughDesc._fields_]
    assert fields == ["max_bounces", "fuzz_limit", "through", "bounces"]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(rt_aov_through_desc));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof(rt_aov_through_desc, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(art.REPO_ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(art.RtAovThroughDesc) == 24
    assert got[1:] == [getattr(art.RtAovThroughDesc, f).offset for f in fields]
    assert list(art.AOV_THROUGH_OUTPUTS) == list(art.AOV_OUTPUTS) + ["through", "bounces"]


def _frame(art, **kw):
    f = art.RtFrameDesc()
    f.nx, f.ny, f.ns, f.gamma, f.tile_rows, f.tile_first, f.tile_stride = 48, 32, 2, 1.0, 32, 0, 1
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _outputs(art, **kw):
    a = art.RtAovDesc()
    a.depth = FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _chain(art, max_bounces=8, fuzz_limit=0.0, **kw):
    t = art.RtAovThroughDesc()
    t.max_bounces, t.fuzz_limit = max_bounces, fuzz_limit
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _call(art, scene, f, a, t):
    L = art.rt_lib()
    ref = lambda x: None if x is None else C.byref(x)   # noqa: E731
    st = L.rt_render_aov_through(scene, ref(f), ref(a), ref(t), 1, None, 1)
    return st, L.rt_last_error_detail().decode()


def test_argument_checks_name_what_failed(art):
    """Every case passes a null scene: the text shows that the check of the frame, the outputs or the chain fired first, with
    no device touched and the scene not looked at."""
    ok_f, ok_a, ok_t = _frame(art), _outputs(art), _chain(art)
    cases = {
        "null f": (None, ok_a, ok_t),
        "null a": (ok_f, None, ok_t),
        "null t": (ok_f, ok_a, None),
        "all outputs null": (ok_f, art.RtAovDesc(), ok_t),
        "max_bounces = -1": (ok_f, ok_a, _chain(art, max_bounces=-1)),
        "max_bounces = 17": (ok_f, ok_a, _chain(art, max_bounces=17)),
        "fuzz_limit < 0": (ok_f, ok_a, _chain(art, fuzz_limit=-0.5)),
        "fuzz_limit nan": (ok_f, ok_a, _chain(art, fuzz_limit=float("nan"))),
        "fuzz_limit inf": (ok_f, ok_a, _chain(art, fuzz_limit=float("inf"))),
        "nx = 0": (_frame(art, nx=0), ok_a, ok_t),
        "ns = 0": (_frame(art, ns=0), ok_a, ok_t),
        "2^32 pixels": (_frame(art, nx=1 << 16, ny=1 << 16, tile_rows=1 << 16), ok_a, ok_t),
        "tile_rows = 0": (_frame(art, tile_rows=0), ok_a, ok_t),
    }
    texts = {}
    for name, (f, a, t) in cases.items():
        st, text = _call(art, None, f, a, t)
        assert st == RT_ERR_INVALID, name
        assert text.startswith("rt_render_aov_through") and "null scene" not in text, (name, text)
        texts[name] = text
    assert "max_bounces" in texts["max_bounces = -1"] and texts["max_bounces = -1"] == texts["max_bounces = 17"]
    assert "fuzz_limit" in texts["fuzz_limit < 0"] and texts["fuzz_limit < 0"] == texts["fuzz_limit nan"] == texts["fuzz_limit inf"]
    st, text = _call(art, None, ok_f, ok_a, ok_t)
    assert st == RT_ERR_INVALID and text.startswith("rt_render_aov_through") and "null scene" in text
    texts["null scene"] = text
    must_differ = ["null f", "null a", "null t", "all outputs null", "max_bounces = 17", "fuzz_limit < 0", "nx = 0", "2^32 pixels",
                   "tile_rows = 0", "null scene"]
    assert len({texts[k] for k in must_differ}) == len(must_differ), texts
    # the limits themselves are accepted, and one output is enough -- of a or of t
    for t in (_chain(art, max_bounces=0), _chain(art, max_bounces=16), _chain(art, fuzz_limit=3.0e38)):
        assert "null scene" in _call(art, None, ok_f, ok_a, t)[1]
    for k in ("through", "bounces"):
        assert "null scene" in _call(art, None, ok_f, art.RtAovDesc(), _chain(art, **{k: FAKE}))[1], k
    # rt_render_aov's own texts are what they were
    L = art.rt_lib()
    assert L.rt_render_aov(None, None, C.byref(ok_a), 1, None, 1) == RT_ERR_INVALID
    assert L.rt_last_error_detail().decode() == "rt_render_aov: null frame description"


def test_through_option(art):
    L = art.rt_lib()
    try:
        for v in (-1, 0, 1, 2):
            assert L.rt_set_option(b"aov_through_lds", v) == 0, v
        for v in (-2, 3):
            assert L.rt_set_option(b"aov_through_lds", v) == RT_ERR_INVALID, v
            assert "aov_through_lds" in L.rt_last_error_detail().decode()
    finally:
        assert L.rt_reset_options() == 0


def test_binding_rejects_malformed_input_before_any_device_work(art):
    ds = art.DeviceScene.__new__(art.DeviceScene)   # no device scene needed: the checks come first
    ds.device, ds._p = 0, C.c_void_p()
    f = _frame(art)
    px = f.nx * f.ny
    bad = [
        lambda: ds.render_aov_through(f, max_bounces=-1),
        lambda: ds.render_aov_through(f, max_bounces=17),
        lambda: ds.render_aov_through(f, max_bounces=2.0),
        lambda: ds.render_aov_through(f, max_bounces=True),
        lambda: ds.render_aov_through(f, fuzz_limit=-1e-3),
        lambda: ds.render_aov_through(f, fuzz_limit=float("nan")),
        lambda: ds.render_aov_through(f, fuzz_limit=float("inf")),
        lambda: ds.render_aov_through(_frame(art, ns=0)),
        lambda: ds.render_aov_through(f, albedo=False, normal=False, depth=False, alpha=False),    # nothing requested
        lambda: ds.render_aov_through(f, out={"colour": np.zeros(px * 3, np.float32)}),            # no such output
        lambda: ds.render_aov_through(f, out={"through": np.zeros(px, np.int32)}),                 # dtype
        lambda: ds.render_aov_through(f, out={"bounces": np.zeros(px, np.float32)}),
        lambda: ds.render_aov_through(f, out={"through": np.zeros(px - 1, np.float32)}),           # size
        lambda: ds.render_aov(f, out={"through": np.zeros(px, np.float32)}),                       # not an output of the plain pass
        lambda: ds.render_denoised(f, max_bounces=99, through=True),
        lambda: ds.render_aov_through(f, through=True, bounces=True),                              # the library: null scene
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")
    assert art.AOV_THROUGH_DEFAULTS["max_bounces"] == 8 and art.AOV_THROUGH_DEFAULTS["fuzz_limit"] >= 0


# ------------------------------------------------------------------------------------------ the restatement of the arithmetic
def test_restated_directions_obey_optics():
    """mirror() and through_glass() in float32 against the law of reflection and Snell's law in float64: unit results, the
    tangential part scaled by the index ratio, the refracted ray on the far side; and total internal reflection exactly where
    sin(theta) e >= 1."""
    rng = np.random.default_rng(5)
    n = rng.normal(size=(4000, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    d = (rng.normal(size=(4000, 3)) * rng.uniform(0.2, 5, (4000, 1))).astype(F)
    ior = rng.choice([0.67, 1.0, 1.5, 2.4], 4000).astype(F)
    u, length = tx.unit(d)
    assert np.allclose(np.linalg.norm(u.astype(np.float64), axis=1), 1, atol=1e-6) and np.allclose(length, np.linalg.norm(d.astype(np.float64), axis=1), rtol=1e-6)
    r = tx.mirror(u, n).astype(np.float64)
    un = (u.astype(np.float64) * n).sum(1)
    assert np.allclose((r * n).sum(1), -un, atol=1e-5) and np.allclose(r + 2 * un[:, None] * n, u, atol=1e-5)
    out, tir = tx.through_glass(d, u, n, ior)
    inside = (d.astype(np.float64) * n).sum(1) > 0
    e = np.where(inside, ior, 1 / ior.astype(np.float64))
    sin_in = np.sqrt(np.maximum(0, 1 - un * un))
    want_tir = sin_in * e >= 1
    sure = np.abs(sin_in * e - 1) > 1e-4
    assert np.array_equal(tir[sure], want_tir[sure]) and tir.any() and (~tir).any() and (tir & ~inside).any() and (tir & inside).any()
    assert np.array_equal(_bits(out[tir]), _bits(tx.mirror(u, n)[tir]))
    t = out[~tir].astype(np.float64)
    assert np.allclose(np.linalg.norm(t, axis=1), 1, atol=1e-5)
    tn = (t * n[~tir]).sum(1)
    assert (np.sign(tn) == np.sign(un[~tir])).all()                               # it goes on through the surface
    tang_in = u[~tir] - un[~tir, None] * n[~tir]
    assert np.allclose(t - tn[:, None] * n[~tir], e[~tir, None] * tang_in, atol=1e-5)   # Snell


# -------------------------------------------------------------------------------------------------- the expectation side
@pytest.fixture(scope="module")
def cases(art, orc):
    return tx.Cases(art, orc)


@pytest.mark.parametrize("key", [tx.SPHERES, tx.GENERAL, tx.GENERAL2])
def test_no_bounce_is_the_plain_expectation(cases, key):
    """max_bounces = 0: normal, depth, alpha and mat are tests/aov_expect.py's, bit for bit; nothing is followed."""
    e = cases.expect(key, ax.NX, ax.NY, 4, 0)
    plain = cases.case(key).expect(4)
    for k in ("normal", "depth", "alpha"):
        assert np.array_equal(_bits(e[k]), _bits(plain[k])), k
    assert np.array_equal(e["mat"], plain["mat"]) and not e["bounces"].any() and not e["through"].any()
    known = ~e["device_needed"].any(axis=2)
    assert np.array_equal(_bits(e["albedo"][known]), _bits(plain["albedo"][known]))


@pytest.mark.parametrize("nx,ny,ns", tx.FRAMES)
def test_spheres_scene_tests_something(cases, nx, ny, ns):
    """The spheres-only scene at the GPU test's frames and fuzz limit: chains of one bounce and of two or more (through a glass
    sphere: in and out), total internal reflection, chains cut by max_bounces at 1 and at 2 and none cut at 8, chains that end
    in a miss, a metal that is followed and one that is not; tints other than white; and the outputs differ from the plain pass's."""
    mats = cases.case(tx.SPHERES).scene.materials()
    metals = mats[mats["kind"] == sg.METAL]
    assert (metals["fuzz"] <= tx.FUZZ_LIMIT).any() and (metals["fuzz"] > tx.FUZZ_LIMIT).any()
    plain = cases.case(tx.SPHERES).expect(ns, nx, ny)
    for mb in tx.BOUNCES:
        e = cases.expect(tx.SPHERES, nx, ny, ns, mb)
        c = e["chain"]
        k = c["k"]
        assert k.max() <= mb and (k == 1).any(), mb
        assert c["metal_followed"].any() and c["metal_unfollowed"].any() and c["tir"].any(), mb
        assert ((k >= 1) & ~c["hit"]).any() and ((k >= 1) & c["hit"]).any(), mb
        assert c["cut"].any() == (mb < 8), mb
        if mb >= 2:
            first = mats["kind"][plain["mats"]]
            assert ((k >= 2) & (first == sg.DIELECTRIC) & (plain["mats"] >= 0)).any(), mb
        assert (c["tint"][c["metal_followed"]] != 1).any()
        assert np.isfinite(e["normal"]).all() and np.isfinite(e["depth"]).all()
        assert (_bits(e["normal"]) != _bits(plain["normal"])).any() and (_bits(e["depth"]) != _bits(plain["depth"])).any()
        far = (k >= 1) & c["hit"]
        assert (c["depth"][far] > plain["t"][far]).all()                                    # the way on only adds to the depth
        assert ((e["through"] > 0) & (e["through"] < 1)).any() == (ns > 1)
        assert (e["bounces"] > 0).any() and (e["mat"][e["bounces"] > 0] != plain["mat"][e["bounces"] > 0]).any()
    assert (cases.expect(tx.SPHERES, nx, ny, ns, 8)["chain"]["k"] > 2).any()


@pytest.mark.parametrize("key", [tx.GENERAL, tx.GENERAL2])
def test_general_scenes_test_something(cases, key):
    """The general scenes: glass is gone through (k >= 2), chains end on quads or behind instances as well as on spheres, and
    some terminal albedo needs a texture (the part of the expectation that leans on DeviceScene.radiance)."""
    e = cases.expect(key, ax.NX, ax.NY, 4, 8)
    c = e["chain"]
    assert (c["k"] == 1).any() and (c["k"] >= 2).any()
    assert (c["metal_followed"] | c["metal_unfollowed"]).any()
    through = c["k"] >= 1
    assert (e["device_needed"] & through).any() and (~e["device_needed"] & through).any()
    if key == tx.GENERAL2:
        assert c["metal_followed"].any() and ((c["k"] >= 1) & ~c["hit"]).any()


def test_fuzz_limit_below_every_fuzz_follows_no_metal(cases):
    """The glass-free scene of the GPU test's fuzz_limit case: it has metals, all with fuzz above the limit used there."""
    scene = cases.case(tx.NO_GLASS).scene
    mats = scene.materials()
    assert not (mats["kind"] == sg.DIELECTRIC).any()
    metals = mats[mats["kind"] == sg.METAL]
    assert len(metals) and (metals["fuzz"] > tx.NO_GLASS_FUZZ_LIMIT).all()
    first = cases.case(tx.NO_GLASS).expect(4)["mats"]
    assert (mats["kind"][first[first >= 0]] == sg.METAL).any()               # and some primary ray lands on one
    e = cases.expect(tx.NO_GLASS, ax.NX, ax.NY, 4, 8, tx.NO_GLASS_FUZZ_LIMIT)
    assert not e["chain"]["k"].any() and e["chain"]["metal_unfollowed"].any()


# ------------------------------------------------------------------------------------------------------------- quality
QUALITY_NX, QUALITY_NY = 96, 64
# RMSE(filtered) / RMSE(noisy) of the colour-factor filter from tools/aov_through_sweep.py: (first-hit guides,
# through guides at the binding's defaults)
MEASURED = {"spheres_plain/1": (0.954, 0.946), "spheres_tex/3": (0.964, 0.972), "general_plain/1": (0.706, 0.702),
            "general_tex/4": (0.838, 0.837), "bouncing": (0.930, 0.934), "final": (0.946, 0.947)}
BEATS_FIRST_HIT = ["spheres_plain/1", "general_plain/1"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aov_through_quality_albedo.npz")


@pytest.mark.parametrize("key", BEATS_FIRST_HIT)
def test_through_guides_beat_first_hit_guides_where_measured(art, orc, key):
    """DESIGN.md 4.11's experiment -- the oracle's 4-spp frame, 96 x 64, the shipped colour-factor filter, against the oracle at
    256 spp and another seed -- with the guides of this pass at the binding's defaults in place of the first-hit ones.  The
    through guides win on the two frames where the sweep shows it (MEASURED: 0.946 < 0.954, 0.702 < 0.706); they do not on
    spheres_tex/3 (0.972 > 0.964) and bouncing (0.934 > 0.930), tie on general_tex/4 and final, and none of those is asserted.
    Normal and depth are the expectation's (oracle only).  The albedo of textured terminals and of the gradient miss term needs
    the device (tests/aov_through_expect.py): it is read from tests/golden, which tools/aov_through_sweep.py --golden wrote, and
    every pixel the host can predict alone must equal that record bit for bit."""
    import denoise_expect as dx
    f = dx.oracle_frame(art, orc, key, ns=4, nx=QUALITY_NX, ny=QUALITY_NY)
    e = tx.expected(f["case"], QUALITY_NX, QUALITY_NY, 4, twin_ds=None, **art.AOV_THROUGH_DEFAULTS)
    albedo = np.load(GOLDEN)[key]
    known = ~e["device_needed"].any(axis=2)
    assert known.any() and (~known).any()
    assert albedo.shape == e["albedo"].shape and np.array_equal(_bits(albedo[known]), _bits(e["albedo"][known]))
    assert np.isfinite(albedo).all() and (e["through"] > 0).any()
    truth, _ = f["oracle"].render(256, gamma=1.0, seed_base=77_000_000_019)
    through = dx.denoise(f["color"], albedo, e["normal"], e["depth"], **art.DENOISE_DEFAULTS)
    first = dx.denoise(f["color"], f["albedo"], f["normal"], f["depth"], **art.DENOISE_DEFAULTS)

    def rmse(a):
        return float(np.sqrt(np.mean((a.astype(np.float64) - truth) ** 2)))
    noisy = rmse(f["color"])
    print(f"{key}: RMSE noisy {noisy:.5f}, first-hit guides {rmse(first) / noisy:.4f}, through guides {rmse(through) / noisy:.4f}")
    assert rmse(through) < rmse(first) < noisy
