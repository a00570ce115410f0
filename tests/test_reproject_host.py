"""rt_scene_set_camera and rt_reproject without a device: the exports, the descriptor's layout against the header, the matrix
against the restatement bit for bit, the argument checks that run before any HIP call, the binding's ValueErrors, make_camera
against the host scene library's own cameras -- and properties of the restatement itself (tests/reproject_expect.py), so that
the GPU parity test (tests/test_reproject.py) cannot agree with a wrong one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reproject_expect as rx
import scene_gen as sg

RT_ERR_INVALID, RT_ERR_NO_DEVICE = 1, 2
FAKE = 0x100000   # never dereferenced: no check looks at what a pointer points to
NEW = ("rt_scene_set_camera", "rt_scene_get_camera", "rt_multi_set_camera", "rt_reproject", "rt_reproject_matrix")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_new_entry_points_are_exported(art):
    for sym in NEW:
        assert sym in art.RT_ABI_SYMBOLS
        assert hasattr(art.rt_lib(), sym)
    assert hasattr(art.host_lib(), "rtw_camera_init")
    assert art.REPROJECT_DEFAULTS == rx.DEFAULTS


def test_reproject_desc_layout_matches_header(art, tmp_path):
    """sizeof and every field offset of rt_reproject_desc as a C compiler lays out include/rt_abi.h."""
    fields = [f for f, _ in art.RtReprojectDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(rt_reproject_desc));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof(rt_reproject_desc, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(art.REPO_ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(art.RtReprojectDesc)
    assert got[1:] == [getattr(art.RtReprojectDesc, f).offset for f in fields]


# ------------------------------------------------------------------------------------------------------------ the matrix
CAMERAS = [((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 1.5, 0.1, 10.0), ((0.3, 2.2, 9.1), (0.0, 0.4, 0.0), 40.0, 48 / 32, 0.0, 9.0),
           ((-4.0, 0.5, -7.0), (1.0, 1.0, 1.0), 75.0, 0.6, 0.2, 3.5), ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0, 1.0, 0.0, 1078.0),
           ((1e-3, 2e-3, 5e-3), (0.0, 0.0, 0.0), 5.0, 2.0, 0.0, 0.004)]


@pytest.mark.parametrize("k", range(len(CAMERAS)))
def test_matrix_equals_the_restatement_bit_for_bit(art, k):
    cam = sg.make_camera(*CAMERAS[k], 0.0, 1.0)
    got, want = art.reproject_matrix(cam), rx.matrix(cam)
    assert want is not None and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    # what the matrix is for: a point a (A + s H + t V) away from the origin maps to (a, a s, a t)
    O, LL, H, V = (np.array(list(x), np.float64) for x in (cam.origin, cam.lower_left_corner, cam.horizontal, cam.vertical))
    a, s, t = 3.25, 0.3, 0.85
    q = a * ((LL - O) + s * H + t * V)
    assert np.allclose(got.astype(np.float64) @ q, [a, a * s, a * t], rtol=1e-5)


def test_matrix_refuses_a_singular_camera(art):
    L = art.rt_lib()
    m = (C.c_float * 9)()
    flat = sg.make_camera(*CAMERAS[0], 0.0, 0.0)
    flat.vertical[:] = flat.horizontal[:]                     # H x V = 0: D == 0
    assert rx.matrix(flat) is None
    assert L.rt_reproject_matrix(C.byref(flat), m) == RT_ERR_INVALID and "singular" in L.rt_last_error_detail().decode()
    tiny = sg.make_camera(*CAMERAS[0], 0.0, 0.0)
    for f in ("horizontal", "vertical"):
        getattr(tiny, f)[:] = [x * 1e-42 for x in getattr(tiny, f)]   # D != 0 in double, the quotients overflow float
    assert rx.matrix(tiny) is None
    assert L.rt_reproject_matrix(C.byref(tiny), m) == RT_ERR_INVALID and "finite" in L.rt_last_error_detail().decode()
    assert L.rt_reproject_matrix(None, m) == RT_ERR_INVALID
    assert L.rt_reproject_matrix(C.byref(flat), None) == RT_ERR_INVALID
    with pytest.raises(ValueError):
        art.reproject_matrix(flat)


# ------------------------------------------------------------------------------------------------- the argument checks
def test_set_camera_checks_name_what_failed(art):
    """Null scene, null camera, a non-finite field, time1 < time0: RT_ERR_INVALID before the scene is looked at (the scene
    pointer here is a fake one) and before any HIP call."""
    L = art.rt_lib()
    good = sg.make_camera(*CAMERAS[1], 0.25, 0.75)

    def changed(**kw):
        c = art.RtCamera.from_buffer_copy(good)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c
    nan, inf = float("nan"), float("inf")
    cases = {"null scene": (None, good), "null camera": (FAKE, None),
             "nan origin": (FAKE, changed(origin=(1, nan))), "inf corner": (FAKE, changed(lower_left_corner=(0, inf))),
             "nan horizontal": (FAKE, changed(horizontal=(2, nan))), "inf vertical": (FAKE, changed(vertical=(0, -inf))),
             "nan u": (FAKE, changed(u=(0, nan))), "nan v": (FAKE, changed(v=(2, nan))), "inf lens": (FAKE, changed(lens_radius=inf)),
             "nan time0": (FAKE, changed(time0=nan)), "inf time1": (FAKE, changed(time1=inf)),
             "time1 < time0": (FAKE, changed(time0=0.5, time1=0.25))}
    texts = {}
    for name, (scene, cam) in cases.items():
        for recal in (0, 1):
            st = L.rt_scene_set_camera(scene, None if cam is None else C.byref(cam), recal)
            text = L.rt_last_error_detail().decode()
            assert st == RT_ERR_INVALID and text.startswith("rt_scene_set_camera"), (name, st, text)
        texts[name] = text
    finite = [k for k in cases if k.split()[0] in ("nan", "inf")]
    assert len({texts[k] for k in finite}) == 1 and "finite" in texts[finite[0]]
    assert len({texts[k] for k in ("null scene", "null camera", finite[0], "time1 < time0")}) == 4, texts
    assert "time1" in texts["time1 < time0"]
    pad = changed(pad=nan)                                   # pad is not a camera field: with a null scene the next check answers
    assert L.rt_scene_set_camera(None, C.byref(pad), 0) == RT_ERR_INVALID
    assert L.rt_scene_get_camera(None, C.byref(good)) == RT_ERR_INVALID
    assert L.rt_scene_get_camera(FAKE, None) == RT_ERR_INVALID
    assert L.rt_multi_set_camera(None, C.byref(good), 0) == RT_ERR_INVALID
    assert L.rt_last_error_detail().decode().startswith("rt_multi_set_camera")
    ds = art.DeviceScene.__new__(art.DeviceScene)            # the binding: a refused camera is a ValueError
    ds.device, ds._p = 0, C.c_void_p(FAKE)
    with pytest.raises(ValueError, match="finite"):
        ds.set_camera(cases["nan origin"][1])
    ds._p = C.c_void_p()


def _desc(art, history=True, **kw):
    d = art.RtReprojectDesc()
    d.nx, d.ny = 37, 29
    d.cur, d.prev = sg.make_camera(*CAMERAS[1], 0.0, 0.0), sg.make_camera(*CAMERAS[0], 0.0, 0.0)
    names = ["color", "depth", "alpha", "out", "out_len"] + (["history", "history_len", "prev_depth", "prev_alpha"] if history else [])
    for k, name in enumerate(names):
        setattr(d, name, FAKE * (k + 1))
    d.alpha_min, d.depth_tol, d.normal_min, d.max_history = 0.5, 0.05, 0.5, 32.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_reproject_checks_name_what_failed(art):
    """Each malformed description is RT_ERR_INVALID with its own text; one that passes every check ends, in a process that has
    initialised no device, at RT_ERR_NO_DEVICE: the checks come before any HIP call."""
    L = art.rt_lib()
    inf, nan = float("inf"), float("nan")
    singular = sg.make_camera(*CAMERAS[0], 0.0, 0.0)
    singular.vertical[:] = singular.horizontal[:]
    cases = {
        "null d": None, "nx = 0": _desc(art, nx=0), "ny < 0": _desc(art, ny=-2), "2^32 pixels": _desc(art, nx=1 << 16, ny=1 << 16),
        "alpha_min = 0": _desc(art, alpha_min=0.0), "alpha_min > 1": _desc(art, alpha_min=1.5), "alpha_min nan": _desc(art, alpha_min=nan),
        "depth_tol < 0": _desc(art, depth_tol=-0.1), "depth_tol > 1": _desc(art, depth_tol=1.01), "depth_tol nan": _desc(art, depth_tol=nan),
        "normal_min < -1": _desc(art, normal_min=-1.5), "normal_min > 1": _desc(art, normal_min=2.0), "normal_min nan": _desc(art, normal_min=nan),
        "max_history < 1": _desc(art, max_history=0.5), "max_history huge": _desc(art, max_history=65537.0), "max_history inf": _desc(art, max_history=inf),
        "null color": _desc(art, color=None), "null depth": _desc(art, depth=None), "null alpha": _desc(art, alpha=None),
        "null out": _desc(art, out=None), "null out_len": _desc(art, out_len=None),
        "history without len": _desc(art, history_len=None), "history without prev_depth": _desc(art, prev_depth=None),
        "history without prev_alpha": _desc(art, prev_alpha=None),
        "len without history": _desc(art, history=False, history_len=FAKE * 9), "prev_alpha without history": _desc(art, history=False, prev_alpha=FAKE * 9),
        "singular prev": _desc(art, prev=singular),
        "out is color": _desc(art, out=FAKE), "out inside history": _desc(art, out=FAKE * 6 + 64), "out_len is depth": _desc(art, out_len=FAKE * 2),
        "motion overlaps out": _desc(art, motion=FAKE * 4 + 128), "motion is alpha": _desc(art, motion=FAKE * 3),
        "out_len inside out": _desc(art, out_len=FAKE * 4 + 4), "out ends in history": _desc(art, out=FAKE * 6 - 64),
    }
    texts = {}
    for name, d in cases.items():
        for on_device in (0, 1):
            st = L.rt_reproject(None if d is None else C.byref(d), on_device, None, 1)
            text = L.rt_last_error_detail().decode()
            assert st == RT_ERR_INVALID and text.startswith("rt_reproject"), (name, on_device, st, text)
        texts[name] = text
    same = [("nx = 0", "ny < 0"), ("alpha_min = 0", "alpha_min > 1", "alpha_min nan"), ("depth_tol < 0", "depth_tol > 1", "depth_tol nan"),
            ("normal_min < -1", "normal_min > 1", "normal_min nan"), ("max_history < 1", "max_history huge", "max_history inf"),
            ("history without len", "history without prev_depth", "history without prev_alpha"),
            ("len without history", "prev_alpha without history")]
    for group in same:
        assert len({texts[k] for k in group}) == 1, group
    distinct = [g[0] for g in same] + ["null d", "2^32 pixels", "null color", "null depth", "null alpha", "null out", "null out_len", "singular prev",
                                       "out is color", "out inside history", "out_len is depth", "motion overlaps out", "motion is alpha",
                                       "out_len inside out"]
    assert len({texts[k] for k in distinct}) == len(distinct), texts
    for name in ("out is color", "out inside history", "out_len is depth", "motion overlaps out", "motion is alpha", "out_len inside out"):
        assert "overlaps" in texts[name], (name, texts[name])
    assert texts["out ends in history"] == texts["out inside history"]   # (an output that starts in front of the buffer it runs into)
    # what passes: with and without a history, every guide, motion, the ends of every range, a non-finite current camera
    wild = sg.make_camera(*CAMERAS[1], 0.0, 0.0)
    wild.origin[0] = nan
    good = [_desc(art), _desc(art, history=False), _desc(art, normal=FAKE * 10, prev_normal=FAKE * 11, prim=FAKE * 12, prev_prim=FAKE * 13, motion=FAKE * 14),
            _desc(art, alpha_min=1.0, depth_tol=0.0, normal_min=-1.0, max_history=1.0), _desc(art, depth_tol=1.0, normal_min=1.0, max_history=65536.0),
            _desc(art, cur=wild)]
    for k, d in enumerate(good):
        if art._initialised_device is None:
            for on_device in (0, 1):
                st = L.rt_reproject(C.byref(d), on_device, None, 1)
                assert st == RT_ERR_NO_DEVICE, (k, on_device, st, L.rt_last_error_detail().decode())
        else:
            st = L.rt_reproject(C.byref(d), 1, None, 1)
            assert st == RT_ERR_INVALID and "device memory" in L.rt_last_error_detail().decode(), (k, st)
    assert 37 * 29 * 12 < FAKE   # (the fake buffers above do not overlap by accident)


def test_binding_rejects_malformed_input_before_any_device_work(art):
    c, z = np.zeros((6, 8, 3), np.float32), np.zeros((6, 8), np.float32)
    cam = sg.make_camera(*CAMERAS[1], 0.0, 0.0)
    hist = dict(history=c, history_len=z, prev_depth=z, prev_alpha=z)
    bad = [
        lambda: art.reproject([[0.0] * 3], z, z, cam, cam),                               # neither numpy nor torch
        lambda: art.reproject(z, z, z, cam, cam),                                          # not (ny, nx, 3)
        lambda: art.reproject(c, None, z, cam, cam),
        lambda: art.reproject(c, z, c, cam, cam),                                          # shape of alpha
        lambda: art.reproject(c, z.astype(np.float64), z, cam, cam),
        lambda: art.reproject(c, z, z, cam, None),
        lambda: art.reproject(c, z, z, cam, cam, history=c),                               # a history without its buffers
        lambda: art.reproject(c, z, z, cam, cam, history_len=z),                           # ... and the other way round
        lambda: art.reproject(c, z, z, cam, cam, prim=z, prev_prim=z, **hist),             # ids are int32
        lambda: art.reproject(c, z, z, cam, cam, out=z, **hist),
        lambda: art.reproject(c, z, z, cam, cam, motion=z, **hist),
        lambda: art.reproject(c, z, z, cam, cam, alpha_min=0.0),
        lambda: art.reproject(c, z, z, cam, cam, depth_tol=float("nan")),
        lambda: art.reproject(c, z, z, cam, cam, normal_min=1.5),
        lambda: art.reproject(c, z, z, cam, cam, max_history=0.0),
        lambda: art.make_camera((0, 0), (0, 0, 0), (0, 1, 0), 40.0, 1.5, 0.0, 1.0),
        lambda: art.make_camera((0, 0, 1), (0, 0, 0), (0, 1, 0), float("nan"), 1.5, 0.0, 1.0),
        lambda: art.make_camera((0, 0, 1), (0, 0, 0), (0, 1, 0), 40.0, 1.5, 0.0, 1.0, 1.0, 0.5),
        lambda: art.TemporalAccumulator(None, art.RtFrameDesc()),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")
    f = art.RtFrameDesc()
    f.nx, f.ny, f.ns, f.gamma, f.tile_rows, f.tile_first, f.tile_stride = 48, 32, 4, 2.0, 4, 0, 2
    with pytest.raises(ValueError):
        art.TemporalAccumulator(None, f)
    f.tile_rows, f.tile_stride = 32, 1
    with pytest.raises(ValueError):
        art.TemporalAccumulator(None, f, depth_tolerance=0.1)   # an unknown threshold


# ------------------------------------------------------------------------------------------------------------ make_camera
@pytest.mark.parametrize("name,args", [
    ("book1", ((13.0, 2.0, 3.0), (0, 0, 0), (0, 1, 0), 20.0, None, 0.1, 10.0)),                  # host/rtw_scenes.cpp, book1_random_scene
    ("checker", ((13.0, 2.0, 3.0), (0, 0, 0), (0, 1, 0), 20.0, None, 0.0, 10.0, 0.0, 1.0))])     # ... checkered_spheres (a shutter)
def test_make_camera_reproduces_a_named_scene_s_camera(art, name, args):
    nx, ny = 200, 120
    hs = art.HostScene(name, nx, ny)
    args = tuple(float(np.float32(nx) / np.float32(ny)) if a is None else a for a in args)
    got, want = art.make_camera(*args), hs.desc.camera
    for f in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v"):
        assert np.array_equal(_bits(np.array(list(getattr(got, f)), np.float32)), _bits(np.array(list(getattr(want, f)), np.float32))), f
    assert (got.lens_radius, got.time0, got.time1) == (want.lens_radius, want.time0, want.time1)
    hs.close()


# ------------------------------------------------------------------------------------------------- the restatement itself
def _plane(nx, ny, depth):
    return dict(color=np.full((ny, nx, 3), 0.25, np.float32), depth=np.full((ny, nx), depth, np.float32), alpha=np.ones((ny, nx), np.float32))


def test_identical_cameras_do_not_move_anything():
    """The same camera twice and a constant-depth plane: every pixel reprojects onto itself -- |motion| <= 1e-3 pixel -- so
    its taps carry its own history: out_len = len + 1, and a constant history blended with a constant frame."""
    nx, ny = 37, 29
    cam = rx.pinhole((0.3, 0.2, 6.0), aspect=nx / ny)
    cur = _plane(nx, ny, 5.5)
    hist = np.full((ny, nx, 3), 0.75, np.float32)
    for n in (1.0, 2.0, 8.0, 16.0, 7.0, 31.0):
        hlen = np.full((ny, nx), n, np.float32)
        out, out_len, motion = rx.reproject(cur["color"], cur["depth"], cur["alpha"], cam, cam, history=hist, history_len=hlen,
                                            prev_depth=cur["depth"], prev_alpha=cur["alpha"])
        assert np.abs(motion).max() <= 1e-3, np.abs(motion).max()
        if n in (1.0, 2.0, 8.0, 16.0):
            # a power of two: every product w * len is exact, so L = len * W in every partial sum and L / W = len exactly
            assert np.array_equal(out_len, hlen + 1)
        else:
            # otherwise four products, three sums (twice) and a quotient each round once: at most 12 roundings of 2^-24
            assert np.abs(out_len - (n + 1)).max() <= 12 * 2.0 ** -24 * n
        assert np.allclose(out, 0.75 + (0.25 - 0.75) / (n + 1), atol=1e-6)
    capped = rx.reproject(cur["color"], cur["depth"], cur["alpha"], cam, cam, history=hist, history_len=np.full((ny, nx), 500.0, np.float32),
                          prev_depth=cur["depth"], prev_alpha=cur["alpha"])[1]
    assert np.array_equal(capped, np.full((ny, nx), 33.0, np.float32))      # max_history = 32
    first = rx.reproject(cur["color"], cur["depth"], cur["alpha"], cam, cam)
    assert np.array_equal(first[0], cur["color"]) and np.array_equal(first[1], np.ones((ny, nx), np.float32))


def test_parallax_of_a_translated_pinhole_camera():
    """A pinhole camera looking down -z at a fronto-parallel plane, then moved by (dx, dy, 0) with its frame: a point at ray
    parameter z (the frame sits at focus_dist = 1, so z is the distance along the axis in units of it) moves by dx / (z W)
    of the frame's width W, i.e. by nx dx / (z |H|) pixels, and likewise in y."""
    nx, ny, z = 64, 48, 4.0
    dx, dy = 0.11, -0.07

    def cam(x, y):
        return sg.make_camera((x, y, 5.0), (x, y, 0.0), 40.0, nx / ny, 0.0, 1.0, 0.0, 0.0)
    cur, prev = cam(0.0, 0.0), cam(dx, dy)
    p = _plane(nx, ny, z)
    hist = np.zeros((ny, nx, 3), np.float32)
    ones = np.ones((ny, nx), np.float32)
    _, out_len, motion = rx.reproject(p["color"], p["depth"], p["alpha"], cur, prev, history=hist, history_len=ones, prev_depth=p["depth"],
                                      prev_alpha=p["alpha"])
    W, Hh = abs(cur.horizontal[0]), abs(cur.vertical[1])
    want = (-dx * nx / (z * W), -dy * ny / (z * Hh))
    assert abs(want[0]) > 1 and abs(want[1]) > 1                        # whole pixels, not a rounding matter
    assert np.abs(motion[..., 0] - want[0]).max() <= 1e-3 and np.abs(motion[..., 1] - want[1]).max() <= 1e-3, (motion[0, 0], want)
    assert (out_len[4:-4, 4:-4] == 2).all() and (out_len == 1).any()    # the interior finds its history, a border strip does not


def test_synthetic_inputs_exercise_every_path():
    """The GPU test's inputs: each rule of the contract decides some pixel."""
    s = rx.synthetic(37, 29, 7)
    b = s["buffers"]
    full = rx.reproject(cur=s["cur"], prev=s["cams"]["near"], **b)
    assert (full[1] > 1).mean() > 0.3 and (full[1] == 1).any()
    assert not np.isfinite(b["depth"]).all() and not np.isfinite(b["prev_depth"]).all() and (b["history_len"] == 0).any()
    assert (b["alpha"] < 0.5).any() and ((b["alpha"] >= 0.5) & (b["alpha"] < 1)).any()
    for off in (dict(normals=False, ids=True), dict(normals=True, ids=False)):
        other = rx.reproject(cur=s["cur"], prev=s["cams"]["near"], **rx.select(b, **off))
        assert not np.array_equal(other[1], full[1]), off                 # each guide rejects taps the others let through
    behind = rx.reproject(cur=s["cur"], prev=s["cams"]["behind"], **b)
    surface = b["alpha"] >= 0.5
    assert (behind[1][surface] == 1).all() and (behind[2][surface] == 0).all()    # a <= 0: no history, no motion
    same = rx.reproject(cur=s["cur"], prev=s["cams"]["same"], **b)
    ok = surface & np.isfinite(b["depth"])
    assert np.abs(same[2][ok]).max() <= 1e-3
    for r in (full, behind, same):
        assert all(x.dtype == np.float32 for x in r)


# ------------------------------------------------------------------------------------------------------------ the CLI
def test_cli_rejects_malformed_orbit_flags(art):
    exe = os.path.join(art.LIB_DIR, "rayTracer")
    base = [exe, "--nx", "16", "--ny", "8", "--ns", "2"]
    for extra in (["--orbit", "3", "30"], ["--temporal"], ["--out", "x"], ["--orbit", "0", "30", "--out", "x"], ["--orbit", "2", "nan", "--out", "x"],
                  ["--orbit", "2", "30", "--out", "x", "--denoise"], ["--orbit", "2", "30", "--out", "x", "--gpus", "2"],
                  ["--orbit", "2", "30", "--out", "x", "--progressive", "1"], ["--orbit", "2", "30", "--out", "x", "--aov", "y"]):
        r = subprocess.run(base + extra, capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--orbit" in r.stderr and r.stdout == b"", (extra, r.returncode, r.stderr)
