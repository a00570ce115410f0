"""rt_render_aov without a device: the export, the descriptor's layout against the header, the argument checks that run before
any HIP call, the option, the binding's ValueErrors -- and the conditions on the oracle side that keep the GPU test
(tests/test_aov.py) from testing nothing, checked on the very scenes and frames it uses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aov_expect as ax
import scene_gen as sg

RT_ERR_INVALID = 1
FAKE = 0x1000   # never dereferenced: every check below fails before a pointer is looked at


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- the library side
def test_render_aov_is_exported(art):
    assert "rt_render_aov" in art.RT_ABI_SYMBOLS
    assert hasattr(art.rt_lib(), "rt_render_aov")


def test_aov_desc_layout_matches_header(art, tmp_path):
    """sizeof and every field offset of rt_aov_desc as a C compiler lays out include/rt_abi.h."""
    fields = [f for f, _ in art.RtAovDesc._fields_]
    assert fields == list(art.AOV_OUTPUTS)
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(rt_aov_desc));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof(rt_aov_desc, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(art.REPO_ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(art.RtAovDesc) == 56
    assert got[1:] == [getattr(art.RtAovDesc, f).offset for f in fields]


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


def _call(art, scene, f, a):
    L = art.rt_lib()
    st = L.rt_render_aov(scene, None if f is None else C.byref(f), None if a is None else C.byref(a), 1, None, 1)
    return st, L.rt_last_error_detail().decode()


def test_argument_checks_name_what_failed(art):
    """Every case passes a null scene: the text shows that the check of the frame or of the outputs fired first, with no
    device touched and the scene not looked at."""
    ok_f, ok_a = _frame(art), _outputs(art)
    cases = {
        "null f": (None, ok_a),
        "null a": (ok_f, None),
        "all outputs null": (ok_f, art.RtAovDesc()),
        "nx = 0": (_frame(art, nx=0), ok_a),
        "ny < 0": (_frame(art, ny=-4), ok_a),
        "ns = 0": (_frame(art, ns=0), ok_a),
        "2^32 pixels": (_frame(art, nx=1 << 16, ny=1 << 16, tile_rows=1 << 16), ok_a),
        "tile_rows = 0": (_frame(art, tile_rows=0), ok_a),
        "tile_stride = 0": (_frame(art, tile_stride=0), ok_a),
        "tile_first < 0": (_frame(art, tile_first=-1), ok_a),
    }
    texts = {}
    for name, (f, a) in cases.items():
        st, text = _call(art, None, f, a)
        assert st == RT_ERR_INVALID, name
        assert text.startswith("rt_render_aov") and "null scene" not in text, (name, text)
        texts[name] = text
    every = art.RtAovDesc(*([FAKE] * 7))
    st, text = _call(art, None, ok_f, every)
    assert st == RT_ERR_INVALID and "null scene" in text
    texts["null scene"] = text
    must_differ = ["null f", "null a", "all outputs null", "nx = 0", "2^32 pixels", "tile_rows = 0", "null scene"]
    assert len({texts[k] for k in must_differ}) == len(must_differ), texts
    assert texts["nx = 0"] == texts["ny < 0"] == texts["ns = 0"]
    assert texts["tile_rows = 0"] == texts["tile_stride = 0"] == texts["tile_first < 0"]
    # one output is enough, whichever it is
    for k in art.AOV_OUTPUTS:
        a = art.RtAovDesc()
        setattr(a, k, FAKE)
        assert "null scene" in _call(art, None, ok_f, a)[1], k


def test_aov_option(art):
    L = art.rt_lib()
    try:
        for v in (-1, 0, 1, 2):
            assert L.rt_set_option(b"aov_lds", v) == 0, v
        for v in (-2, 3):
            assert L.rt_set_option(b"aov_lds", v) == RT_ERR_INVALID, v
            assert "aov_lds" in L.rt_last_error_detail().decode()
    finally:
        assert L.rt_reset_options() == 0
    assert L.rt_set_option(b"aov_lds", -1) == 0


def test_binding_rejects_malformed_input_before_any_device_work(art):
    ds = art.DeviceScene.__new__(art.DeviceScene)   # no device scene needed: the checks come first
    ds.device, ds._p = 0, C.c_void_p()
    f = _frame(art)
    px = f.nx * f.ny
    bad = [
        lambda: ds.render_aov(_frame(art, nx=0)),
        lambda: ds.render_aov(_frame(art, ns=0)),
        lambda: ds.render_aov(_frame(art, tile_rows=0)),
        lambda: ds.render_aov(f, albedo=False, normal=False, depth=False, alpha=False),          # nothing requested
        lambda: ds.render_aov(f, out={}),
        lambda: ds.render_aov(f, out={"colour": np.zeros(px * 3, np.float32)}),                  # no such output
        lambda: ds.render_aov(f, out={"depth": np.zeros(px - 1, np.float32)}),                   # size
        lambda: ds.render_aov(f, out={"depth": np.zeros(px, np.float64)}),                       # dtype
        lambda: ds.render_aov(f, out={"mat": np.zeros(px, np.float32)}),
        lambda: ds.render_aov(f, out={"albedo": np.zeros((f.ny, f.nx, 6), np.float32)[:, :, ::2]}),   # not contiguous
        lambda: ds.render_aov(f, out={"depth": [0.0] * px}),                                     # neither numpy nor torch
        lambda: ds.render_aov(f),                                                                # the library: null scene
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")


# -------------------------------------------------------------------------------------------------------- the oracle side
@pytest.fixture(scope="module")
def cases(art, orc):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = ax.Case(art, orc, key)
        return cache[key]
    return get


def test_twin_materials():
    mats = np.zeros(5, sg.art.MATERIAL_DTYPE)
    mats["kind"] = [sg.LAMBERTIAN, sg.METAL, sg.DIELECTRIC, sg.LIGHT, sg.ISOTROPIC]
    mats["tex"] = [3, 2, 1, -1, 0]
    mats["albedo"] = np.arange(15).reshape(5, 3) / 16
    mats["fuzz"], mats["ior"] = 0.5, 1.5
    t = ax.twin_materials(mats)
    assert (t["kind"] == sg.LIGHT).all()
    assert list(t["tex"]) == [3, -1, -1, -1, 0]
    assert np.array_equal(t["albedo"][[0, 1, 3, 4]], mats["albedo"][[0, 1, 3, 4]]) and (t["albedo"][2] == 1).all()
    assert mats["kind"][0] == sg.LAMBERTIAN          # the original is left alone


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("key", ax.PARITY)
def test_parity_scenes_test_something(cases, key, ns):
    """The scenes and frames of tests/test_aov.py.  The identity the expectation rests on: the twin's render sends exactly
    one ray per sample (no path goes on), and the t its ray sample records -- the twin's walk -- equals, bit for bit, the t
    OracleScene.trace finds for those rays in the original scene.  And the frame is not empty: at most half of the samples
    miss, the first hits land on at least three material kinds, and -- in every scene that has a textured material at all;
    spheres_plain, media_many, limits and cornell_smoke have none by construction -- some hit is on a textured lambertian,
    isotropic or light material, so that albedo comes from a texture."""
    c = cases(key)
    e = c.expect(ns)
    n = ax.NX * ax.NY * ns
    assert e["counters"]["rays"] == e["counters"]["samples"] == n == len(e["rays"])
    assert np.array_equal(_bits(e["t"]), _bits(e["twin_t"]))
    hit = e["mats"] >= 0
    assert (~hit).mean() <= 0.5, (key, float((~hit).mean()))
    mats = c.scene.materials()
    first = mats[e["mats"][hit]]
    assert len(np.unique(first["kind"])) >= 3, (key, np.unique(first["kind"]))
    if (mats["tex"] >= 0).any():
        assert ((first["tex"] >= 0) & (first["kind"] != sg.METAL) & (first["kind"] != sg.DIELECTRIC)).any(), key
    for k in ("albedo", "normal", "depth", "alpha"):
        assert np.isfinite(e[k]).all(), k
    assert ((e["alpha"] > 0) == (e["depth"] > 0)).all()
    if ns == 3:   # pixels on a silhouette: coverage strictly between 0 and 1, which no single sample can give
        assert ((e["alpha"] > 0) & (e["alpha"] < 1)).any(), key


def test_parity_set_covers_every_texture_level_and_both_families():
    """Between them the parity scenes reach every instantiation family of the kernel: spheres-only and general, and a
    textured hit under solid / checker textures only (level 1) and under procedural and image textures (level 2)."""
    import accelerated_ray_tracer_amd as art
    seen = set()
    for key in ax.PARITY:
        s = ax.load_scene(art, key)
        prim = s.nodes()["prim"]
        spheres_only = bool(((prim[prim >= 0] >> 28) == sg.SPHERE).all()) and s.desc.n_quads == 0 and s.desc.n_media == 0
        tex = s.materials()["tex"]
        level = 0
        if (tex >= 0).any():
            kinds = np.frombuffer((C.c_char * (64 * s.desc.n_textures)).from_address(s.desc.textures), sg.TEXTURE_DTYPE)["kind"]
            level = 2 if np.isin(kinds, [sg.T_IMAGE, sg.T_NOISE, sg.T_NOODLE, sg.T_FELT, sg.T_UVOFF]).any() else 1
        seen.add((spheres_only, level))
    assert seen == {(so, lv) for so in (True, False) for lv in (0, 1, 2)}, seen
