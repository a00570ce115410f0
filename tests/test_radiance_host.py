"""rt_radiance_rays without a device: the export, the batch layout against the header, the argument checks that run before
any HIP call, the option, the binding's ValueErrors -- and the expectation helper (tests/radiance_expect.py) anchored on the
existing oracle, with the conditions that keep the GPU test's ray sets from testing nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import radiance_expect as rx
import scene_gen as sg

RT_ERR_INVALID = 1
FAKE = 0x1000   # never dereferenced: every check below fails before a pointer is looked at
FLT_MAX = np.float32(np.finfo(np.float32).max)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_radiance_rays_is_exported(art):
    assert "rt_radiance_rays" in art.RT_ABI_SYMBOLS
    assert hasattr(art.rt_lib(), "rt_radiance_rays")


def test_radiance_batch_layout_matches_header(art, tmp_path):
    """sizeof and every field offset of rt_radiance_batch as a C compiler lays out include/rt_abi.h."""
    fields = [f for f, _ in art.RtRadianceBatch._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(rt_radiance_batch));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof(rt_radiance_batch, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(art.REPO_ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(art.RtRadianceBatch) == 88
    assert got[1:] == [getattr(art.RtRadianceBatch, f).offset for f in fields]


def _batch(art, **kw):
    b = art.RtRadianceBatch()
    b.n, b.origins, b.directions, b.ns, b.rgb_out = 4, FAKE, FAKE, 1, FAKE
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _call(art, scene, batch):
    L = art.rt_lib()
    st = L.rt_radiance_rays(scene, None if batch is None else C.byref(batch), None, 1)
    return st, L.rt_last_error_detail().decode()


def test_argument_checks_name_what_failed(art):
    """Every case passes a null scene: the text shows that the batch check fired first, with no device touched."""
    cases = {
        "null batch": None,
        "n < 0": _batch(art, n=-1),
        "ns = 0": _batch(art, ns=0),
        "ns < 0": _batch(art, ns=-3),
        "ns too large": _batch(art, ns=(1 << 20) + 1),
        "null origins": _batch(art, origins=None),
        "null directions": _batch(art, directions=None),
        "null rgb_out": _batch(art, rgb_out=None),
    }
    texts = {}
    for name, b in cases.items():
        st, text = _call(art, None, b)
        assert st == RT_ERR_INVALID, name
        assert text.startswith("rt_radiance_rays") and "null scene" not in text, (name, text)
        texts[name] = text
    st, text = _call(art, None, _batch(art, ns=1 << 20, seeds=FAKE, times=FAKE, rays_out=FAKE))
    assert st == RT_ERR_INVALID and "null scene" in text
    texts["null scene"] = text
    must_differ = ["null batch", "n < 0", "ns = 0", "null origins", "null rgb_out", "null scene"]
    assert len({texts[k] for k in must_differ}) == len(must_differ), texts
    assert texts["ns = 0"] == texts["ns < 0"] == texts["ns too large"]
    assert texts["null origins"] == texts["null directions"]


def test_radiance_option(art):
    L = art.rt_lib()
    try:
        for v in (-1, 0, 1, 2):
            assert L.rt_set_option(b"radiance_lds", v) == 0, v
        for v in (-2, 3):
            assert L.rt_set_option(b"radiance_lds", v) == RT_ERR_INVALID, v
            assert "radiance_lds" in L.rt_last_error_detail().decode()
    finally:
        assert L.rt_reset_options() == 0


def test_binding_rejects_malformed_input_before_any_device_work(art):
    import torch
    ds = art.DeviceScene.__new__(art.DeviceScene)   # no device scene needed: the checks come first
    ds.device, ds._p = 0, C.c_void_p()
    o = np.zeros((4, 3), np.float32)
    tm = np.zeros(4, np.float32)
    seeds = np.arange(4, dtype=np.uint64)
    ok = dict(background=(0, 0, 0), gradient=False)
    bad = [
        lambda: ds.radiance(np.zeros((4, 4), np.float32), o, **ok),            # shape
        lambda: ds.radiance(o, None, **ok),                                     # directions missing
        lambda: ds.radiance(o, o[:3], **ok),                                    # length
        lambda: ds.radiance(o.astype(np.float64), o, **ok),                     # dtype
        lambda: ds.radiance(o, o, tm.astype(np.float64), **ok),
        lambda: ds.radiance(o, o, tm[:2], **ok),
        lambda: ds.radiance(o, o, seeds=seeds.astype(np.int32), **ok),          # seeds are 64-bit
        lambda: ds.radiance(o, o, seeds=seeds[:3], **ok),
        lambda: ds.radiance(o, o, ns=0, **ok),
        lambda: ds.radiance(o, o, ns=(1 << 20) + 1, **ok),
        lambda: ds.radiance(o, o, ns=2.0, **ok),
        lambda: ds.radiance(o, o, seed_base=-1, **ok),
        lambda: ds.radiance(o, o, background=(0, 0), gradient=False),
        lambda: ds.radiance(o, torch.zeros((4, 3)), **ok),                      # numpy mixed with a tensor
        lambda: ds.radiance(torch.zeros((4, 3)), torch.zeros((4, 3)), **ok),    # CPU tensors
        lambda: ds.radiance([[0, 0, 0]], o, **ok),                              # neither numpy nor torch
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {k} was accepted")


# ----------------------------------------------------------------------------- the helper, anchored on the existing oracle
def _probe_rays(orc, art, name, n=600):
    hs = rx.load_scene(art, name)
    whole = orc.OracleScene.from_host(hs)
    o, p, tm = rx.ray_set(hs, whole, n)
    t, _, _, _, mat = whole.trace(o, rx.directions(o, p), tm)
    return hs, o, p, tm, t, mat


@pytest.mark.parametrize("name", ["simple_light", "cornell"])
def test_expect_gives_the_background_for_missing_rays(art, orc, name):
    """Rays that OracleScene.trace says miss: with a constant background the expectation is that background exactly (sums of
    up to four of these values and the scaling by 1/ns are exact) and one world->hit call per sample."""
    hs, o, p, tm, t, mat = _probe_rays(orc, art, name)
    miss = np.flatnonzero(t == FLT_MAX)[:40]
    assert len(miss) >= 10, len(miss)
    bg = np.array([0.25, 0.5, 0.75], np.float32)
    for ns in (1, 4):
        rgb, rays = rx.expect(orc, hs, o[miss], p[miss], tm[miss], rx.explicit_seeds(len(miss)), ns, bg, 0)
        assert np.array_equal(_bits(rgb), _bits(np.broadcast_to(bg, rgb.shape)))
        assert (rays == ns).all()


@pytest.mark.parametrize("name", ["simple_light", "cornell"])
def test_expect_gives_the_light_for_rays_that_end_on_one(art, orc, name):
    """Rays whose first hit is a solid diffuse light: the light's colour (small integers here: the sum over the samples is
    exact) and one world->hit call per sample."""
    hs, o, p, tm, t, mat = _probe_rays(orc, art, name, 1500)
    mats = hs.materials()
    light = np.flatnonzero((t < FLT_MAX) & (mats["kind"][np.maximum(mat, 0)] == sg.LIGHT) & (mats["tex"][np.maximum(mat, 0)] < 0))[:40]
    assert len(light) >= 5, len(light)
    for ns in (1, 4):
        rgb, rays = rx.expect(orc, hs, o[light], p[light], tm[light], rx.default_seeds(len(light)), ns, (0.25, 0.5, 0.75), 0)
        want = mats["albedo"][mat[light]]
        assert (want == np.round(want)).all() and (want > 0).all()
        assert np.array_equal(_bits(rgb), _bits(want))
        assert (rays == ns).all()


@pytest.fixture(scope="module")
def cases(art, orc):
    cache = {}

    def get(key, n):
        if (key, n) not in cache:
            cache[(key, n)] = rx.Case(art, orc, key, n)
        return cache[(key, n)]
    return get


@pytest.mark.parametrize("key,n", rx.PARITY + [rx.LARGE])
def test_parity_ray_sets_test_something(cases, key, n):
    """The ray sets of tests/test_radiance.py: no NaN, at most half of the queries are pure misses (rays == ns), the first hits
    cover at least three materials where the scene has that many, some query bounces (more than 3 * ns rays), and the two
    seedings give different results."""
    c = cases(key, n)
    assert c.n == n == len(c.o) == len(c.d) == len(c.tm)
    t, _, _, _, mat = c.whole.trace(c.o, c.d, c.tm)
    n_mat = c.scene.desc.n_materials
    assert len(np.unique(mat[t < FLT_MAX])) >= min(3, n_mat), (key, np.unique(mat))
    for ns in (1, 4):
        rgb, rays = c.expect("default", ns)
        assert not np.isnan(rgb).any()
        assert (rays >= ns).all() and (rays <= 50 * ns).all()
        assert (rays == ns).mean() <= 0.5, (key, ns, float((rays == ns).mean()))
        assert (rays > 3 * ns).any()
    assert not np.array_equal(_bits(c.expect("default", 4)[0]), _bits(c.expect("explicit", 4)[0]))
