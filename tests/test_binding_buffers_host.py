"""The binding's one rule for buffers, streams and refusals, without a device: every buffer argument of every entry point
gets every defect the rule knows, and each is a ValueError that names the argument before anything reaches the library.

The device methods run on a DeviceScene made with __new__ and a null scene: a call that passes every Python check ends in the
library's own refusal of the null scene (or, for the module-level denoise / reproject, at the device when one is
initialised), never in a launch."""
import ctypes as C

import numpy as np
import pytest
import torch

NX, NY, RAYS, RECORDS = 5, 3, 3, 2
RGB, ONE, MOTION = (NY, NX, 3), (NY, NX), (NY, NX, 2)
POINTER = 1 << 20                      # stands for device memory: the null scene is refused before anything looks at it
NOT_A_POINTER = [("True", True), ("3.7", 3.7), ("a string", "x")]


def _scene(art):
    ds = art.DeviceScene.__new__(art.DeviceScene)   # no device scene needed: the checks come first
    ds.device, ds._p = 0, C.c_void_p()
    return ds


def _frame(art):
    f = art.RtFrameDesc()
    f.nx, f.ny, f.ns, f.gamma, f.tile_rows, f.tile_first, f.tile_stride = NX, NY, 4, 2.0, NY, 0, 1
    return f


def _wider(a):
    return np.zeros(a.shape[:-1] + (a.shape[-1] + 1,), a.dtype)


def _strided(a):
    return np.zeros(a.shape[:-1] + (2 * a.shape[-1],), a.dtype)[..., ::2]


def _other_dtype(a):
    return a.astype({np.dtype(np.float32): np.float64, np.dtype(np.int32): np.float32, np.dtype(np.int64): np.int32}[a.dtype])


def _array_defects(good, anchor=False, counted=False, strided_ok=False):
    """(label, value) for every defect of an array argument whose good value is `good`.  An anchor decides whether the call
    is a host or a device call, so a CPU tensor there is a device call on the wrong device: tests/test_binding_buffers.py."""
    bad = [("a list", good.tolist()), ("wrong dtype", _other_dtype(good)),
           ("wrong size", np.zeros(good.size + 1, good.dtype) if counted else _wider(good))]
    if not anchor:
        bad.append(("a CPU tensor", torch.from_numpy(good.copy())))
    if not strided_ok:
        bad.append(("strided", _strided(good)))
        if good.ndim > 1:
            bad.append(("Fortran-ordered", np.asfortranarray(good)))
    return bad


def _table_defects(good, other, prev=False):
    bad = [("a list", good.tolist()), ("a CPU tensor", torch.zeros((len(good), good.dtype.itemsize // 4))),
           ("two-dimensional", good.reshape(1, -1)), ("another structured dtype", np.zeros(len(good), other))]
    if prev:
        bad.append(("another length", np.zeros(len(good) + 1, good.dtype)))
    return bad


def _refusal(call, names):
    """None when `call` raises a ValueError that starts with one of `names` and a colon, else what it did instead."""
    try:
        call()
    except ValueError as e:
        return None if any(str(e).startswith(n + ": ") for n in names) else f"ValueError without the name: {e}"
    except Exception as e:   # noqa: BLE001
        return f"{type(e).__name__}: {e}"
    return "accepted"


def _passes_the_binding(call):
    """`call` gets past every Python check: it returns, or what stops it is the library (a detail that starts with the entry's
    name, or an RtError) or torch finding no device to copy to -- never a ValueError that names an argument."""
    try:
        call()
    except ValueError as e:
        assert str(e).startswith("rt_"), f"refused by the binding: {e}"
    except RuntimeError:
        pass


def _check_all(cases):
    """cases: (label, call, names).  Every one must be refused by name; all that are not are reported together."""
    wrong = [f"{label}: {r}" for label, call, names in cases for r in [_refusal(call, names)] if r is not None]
    assert not wrong, "\n".join(wrong)


# --------------------------------------------------------------------------------------------------- denoise, reproject
def _denoise_args():
    rgb, one = np.zeros(RGB, np.float32), np.zeros(ONE, np.float32)
    return dict(color=rgb, albedo=rgb.copy(), normal=rgb.copy(), depth=one, out=rgb.copy(), variance=one.copy(), variance_out=one.copy())


def test_denoise(art):
    good = _denoise_args()
    _passes_the_binding(lambda: art.denoise(**good))
    cases = [(f"{k} {label}", lambda k=k, v=v: art.denoise(**dict(good, **{k: v})), (k,))
             for k in good for label, v in _array_defects(good[k], anchor=k == "color")]
    _check_all(cases)
    with pytest.raises(ValueError, match="^workspace: "):
        art.denoise(good["color"], workspace=np.zeros(1 << 16, np.uint8))


def _reproject_args(art):
    rgb, one, ids = np.zeros(RGB, np.float32), np.zeros(ONE, np.float32), np.zeros(ONE, np.int32)
    cam = art.make_camera((0, 0, 1), (0, 0, 0), (0, 1, 0), 40.0, NX / NY, 0.0, 1.0)
    planes = dict(color=rgb, depth=one, alpha=one, normal=rgb, prim=ids, history=rgb, history_len=one, prev_depth=one, prev_alpha=one,
                  prev_normal=rgb, prev_prim=ids, out=rgb, out_len=one, motion=np.zeros(MOTION, np.float32), inst=ids, prev_inst=ids)
    planes = {k: v.copy() for k, v in planes.items()}
    tables = dict(spheres=art.SPHERE_DTYPE, prev_spheres=art.SPHERE_DTYPE, media=art.MEDIUM_DTYPE, instances=art.INSTANCE_DTYPE,
                  prev_instances=art.INSTANCE_DTYPE, quads=art.QUAD_DTYPE, prev_quads=art.QUAD_DTYPE)
    tables = {k: np.zeros(RECORDS, d) for k, d in tables.items()}
    return dict(cur=cam, prev=cam), planes, tables


def test_reproject(art):
    cams, planes, tables = _reproject_args(art)
    good = dict(cams, **planes, **tables)
    _passes_the_binding(lambda: art.reproject(**good))
    _passes_the_binding(lambda: art.reproject(**dict(good, **{k: np.repeat(v, 2)[::2] for k, v in tables.items()})))   # made contiguous
    _passes_the_binding(lambda: art.reproject(**dict(good, media=np.zeros(0, art.MEDIUM_DTYPE))))
    cases = [(f"{k} {label}", lambda k=k, v=v: art.reproject(**dict(good, **{k: v})), (k,))
             for k in planes for label, v in _array_defects(planes[k], anchor=k == "color")]
    cases += [(f"{k} {label}", lambda k=k, v=v: art.reproject(**dict(good, **{k: v})), (k,))
              for k in tables for label, v in _table_defects(tables[k], art.NODE_DTYPE, prev=k.startswith("prev_"))]
    _check_all(cases)


# ---------------------------------------------------------------------------------------- the frame entries of a scene
@pytest.mark.parametrize("through", [False, True])
def test_aov(art, through):
    ds, f = _scene(art), _frame(art)
    table = art.AOV_THROUGH_OUTPUTS if through else art.AOV_OUTPUTS
    call = ds.render_aov_through if through else ds.render_aov
    good = {k: np.zeros(RGB if ch == 3 else ONE, dtype) for k, (ch, dtype) in table.items()}
    _passes_the_binding(lambda: call(f, out=good))
    _passes_the_binding(lambda: call(f, out={k: v.reshape(-1) for k, v in good.items()}))          # the element count is the rule
    cases = []
    for k in good:
        for label, v in _array_defects(good[k], counted=True):
            # a value that is no array makes the dict a device call whose other values are no tensors: `out` is what is wrong
            names = (k, "out") if label in ("a list", "a CPU tensor") else (k,)
            cases.append((f"{k} {label}", lambda k=k, v=v: call(f, out=dict(good, **{k: v})), names))
    cases.append(("all CPU tensors", lambda: call(f, out={k: torch.from_numpy(v) for k, v in good.items()}), (next(iter(good)),)))
    _check_all(cases)


@pytest.mark.parametrize("entry", ["render_variance", "render_adaptive"])
def test_frame_with_a_second_plane(art, entry):
    """render_variance(out, variance_out) and render_adaptive(out, spp_out): numpy arrays, or device memory as tensors or
    integer pointers.  render_adaptive once took anything int() takes as a pointer -- out=True went to the library as the
    address 1; it now has render_variance's rule."""
    ds, f = _scene(art), _frame(art)
    second, dtype = ("variance_out", np.float32) if entry == "render_variance" else ("spp_out", np.int32)
    good = {"out": np.zeros(RGB, np.float32), second: np.zeros(ONE, dtype)}

    def call(**kw):
        method, args = (ds.render_variance, (f, 2)) if entry == "render_variance" else (ds.render_adaptive, (f, 2, 4, 0.1))
        return method(*args, **kw)
    _passes_the_binding(lambda: call(**good))
    _passes_the_binding(lambda: call(**{k: v.reshape(-1) for k, v in good.items()}))
    _passes_the_binding(lambda: call(**{"out": POINTER, second: 2 * POINTER}))
    _passes_the_binding(lambda: call(**{"out": np.int64(POINTER), second: 2 * POINTER}))
    cases = []
    for k in good:
        other = "out" if k == second else second
        for label, v in _array_defects(good[k], anchor=k == "out", counted=True):
            # beside a bad value that is no array the other argument is device memory, so that the kinds agree
            rest = {other: POINTER} if label in ("a list", "a CPU tensor") else {other: good[other]}
            cases.append((f"{k} {label}", lambda k=k, v=v, rest=rest: call(**{k: v}, **rest), (k,)))
        cases += [(f"{k} {label}", lambda k=k, v=v, other=other: call(**{k: v, other: POINTER}), (k,)) for label, v in NOT_A_POINTER]
    _check_all(cases)


# ------------------------------------------------------------------------------------------------------- trace, radiance
def _rays():
    o = np.zeros((RAYS, 3), np.float32)
    d = np.tile(np.float32([0, 0, -1]), (RAYS, 1))
    return dict(origins=o, directions=d, times=np.zeros(RAYS, np.float32))


@pytest.mark.parametrize("entry", ["trace", "radiance"])
def test_ray_queries(art, entry):
    ds = _scene(art)
    good = _rays()
    if entry == "trace":
        good["tmax"] = np.full(RAYS, 10.0, np.float32)
        call = ds.trace
    else:
        good["seeds"] = np.arange(RAYS, dtype=np.int64)
        call = lambda **kw: ds.radiance(background=[0.0, 0.0, 0.0], gradient=False, **kw)   # noqa: E731
    _passes_the_binding(lambda: call(**good))
    for k, v in good.items():                         # a strided or Fortran-ordered input is copied, not refused
        _passes_the_binding(lambda: call(**dict(good, **{k: _strided(v)})))
    _passes_the_binding(lambda: call(**dict(good, origins=np.asfortranarray(good["origins"]))))
    if entry == "radiance":
        _passes_the_binding(lambda: call(**dict(good, seeds=good["seeds"].astype(np.uint64))))
    cases = [(f"{k} {label}", lambda k=k, v=v: call(**dict(good, **{k: v})), (k,))
             for k in good for label, v in _array_defects(good[k], anchor=k == "origins", strided_ok=True)]
    _check_all(cases)


# --------------------------------------------------------------------------------------------------------------- updates
@pytest.mark.parametrize("kind", ["spheres", "instances", "quads"])
def test_updates(art, kind):
    ds = _scene(art)
    dtype = {"spheres": art.SPHERE_DTYPE, "instances": art.INSTANCE_DTYPE, "quads": art.QUAD_DTYPE}[kind]
    call = getattr(ds, "update_" + kind)
    good = np.zeros(RECORDS, dtype)
    _passes_the_binding(lambda: call(good))
    _passes_the_binding(lambda: call(np.repeat(good, 2)[::2]))                                  # made contiguous
    _check_all([(label, lambda v=v: call(v), (kind,)) for label, v in _table_defects(good, art.NODE_DTYPE)])
    _check_all([("indices of another length", lambda: call(good, indices=[0]), ("indices",)),
                ("a stream with host records", lambda: call(good, stream=1234), ("stream",))])


# ------------------------------------------------------------------------------------------------- _status, _stream_arg
def test_status_turns_a_refusal_into_a_value_error(art):
    L = art.rt_lib()
    flat = art.make_camera((0, 0, 1), (0, 0, 0), (0, 1, 0), 40.0, NX / NY, 0.0, 1.0)
    flat.vertical[:] = flat.horizontal[:]
    m = (C.c_float * 9)()
    st = L.rt_reproject_matrix(C.byref(flat), m)
    assert st == 1
    with pytest.raises(ValueError, match="^rt_reproject_matrix.*singular") as e:
        art._status(st, "rt_reproject_matrix")
    assert str(e.value) == L.rt_last_error_detail().decode()
    art._status(0, "rt_reproject_matrix")
    with pytest.raises(art.RtError, match="^an entry: ") as e:          # any other status: what _check raises
        art._status(2, "an entry")
    assert not isinstance(e.value, ValueError)
    with pytest.raises(art.RtError) as c:
        art._check(2, "an entry")
    assert str(c.value) == str(e.value)


def test_stream_arg(art):
    class Stream:
        cuda_stream = 0x5678

    class NullStream:
        cuda_stream = 0
    assert art._stream_arg(0) is None and art._stream_arg(None) is None and art._stream_arg(NullStream()) is None
    for given, want in ((1234, 1234), (np.int64(1234), 1234), (Stream(), 0x5678)):
        p = art._stream_arg(given)
        assert isinstance(p, C.c_void_p) and p.value == want


# ---------------------------------------------------------------------------------------------------- the public surface
PUBLIC = """RtError RtCamera RtSceneDesc RtFrameDesc RtStats RtRayBatch RtRadianceBatch RtAovDesc RtAovThroughDesc RtDenoiseDesc
RtAdaptiveDesc RtVarianceDesc RtDenoiseVarianceDesc RtReprojectDesc RtReprojectMotionDesc RtReprojectInstanceDesc RtReprojectQuadDesc
RtSphereUpdate RtInstanceUpdate RtQuadUpdate prim_kind prim_index build host_lib rt_lib load_ppm default_texture HostScene
HostScene.nodes HostScene.spheres HostScene.materials HostScene.quads HostScene.instances HostScene.media HostScene.leaf_order
HostScene.frame HostScene.close init set_option reset_options denoise_workspace_bytes denoise make_camera reproject_matrix reproject
refit_nodes refit_instances refit_quads quad_record box_records instance_record DeviceScene DeviceScene.set_camera DeviceScene.camera
DeviceScene.update_spheres DeviceScene.update_instances DeviceScene.update_quads DeviceScene.spheres DeviceScene.instances
DeviceScene.quads DeviceScene.debug_quads DeviceScene.cost_map DeviceScene.set_cost_map DeviceScene.render DeviceScene.trace
DeviceScene.radiance DeviceScene.render_aov DeviceScene.render_aov_through DeviceScene.render_denoised DeviceScene.render_variance
DeviceScene.render_adaptive DeviceScene.adaptive_passes DeviceScene.progressive DeviceScene.walk_info DeviceScene.finish
DeviceScene.close ProgressiveFrame ProgressiveFrame.render ProgressiveFrame.close TemporalAccumulator TemporalAccumulator.reset
TemporalAccumulator.push MultiScene MultiScene.set_camera MultiScene.update_spheres MultiScene.update_instances
MultiScene.update_quads MultiScene.render MultiScene.close plan_walk_array regroup_leaves row_owner local_rows_to_global write_ppm"""


def test_the_public_names_are_all_there(art):
    """Every function, class and method the binding offered before its buffer handling was unified, by name."""
    missing = []
    for name in PUBLIC.split():
        obj = art
        for part in name.split("."):
            obj = getattr(obj, part, None)
        if not callable(obj):
            missing.append(name)
    assert not missing, missing
    ref = np.int32([(art.RT_PRIM_QUAD << 28) | 5, -1])
    assert art.prim_kind(ref).tolist() == [art.RT_PRIM_QUAD, 15] and art.prim_index(ref)[0] == 5
