"""The binding's buffer rule on device tensors: what tests/test_binding_buffers_host.py cannot isolate without a device -- a
wrong dtype, size or layout of a tensor on the device, a tensor on the CPU in every entry's anchor, an array among tensors.

Nothing here provokes anything: every bad call is refused in Python before any launch, and the scene methods run on a null
scene, so a call the binding wrongly let through would be refused by the library, not launched.  (Good calls on a side
stream are test_trace_rays.py::test_torch_path, test_radiance.py::test_torch_path and
test_update_spheres.py::test_device_resident_records[True].)"""
import numpy as np
import pytest
import torch

import test_binding_buffers_host as host
from test_binding_buffers_host import ONE, RECORDS, RGB

pytestmark = pytest.mark.gpu


def _cuda(x):
    return torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x


def _tensor_defects(good, anchor=False, counted=False, strided_ok=False, among_arrays=True):
    shape = tuple(good.shape)
    bad = [("wrong dtype", good.int() if good.dtype == torch.int64 else good.float() if good.dtype == torch.int32 else good.double()),
           ("wrong size", torch.zeros(good.numel() + 1 if counted else shape[:-1] + (shape[-1] + 1,), dtype=good.dtype, device=good.device)),
           ("a CPU tensor", good.cpu())]
    if not anchor and among_arrays:
        bad.append(("a numpy array", good.cpu().numpy()))
    if not strided_ok:
        bad.append(("strided", torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=good.dtype, device=good.device)[..., ::2]))
    return bad


def _table_defects(good, dtype=None, prev=False):
    n, words = good.shape
    bad = [("wrong width", good[:, :-1].contiguous()), ("an 8-byte dtype", good.double()), ("one-dimensional", good.reshape(-1)),
           ("strided", torch.zeros((n, 2 * words), device=good.device)[:, :words]), ("transposed", good.t()), ("a CPU tensor", good.cpu())]
    if dtype is not None:
        bad.append(("a numpy array", np.zeros(n, dtype)))
    if prev:
        bad.append(("another length", torch.zeros((n + 1, words), device=good.device)))
    return bad


def test_denoise(gpu):
    good = {k: _cuda(v) for k, v in host._denoise_args().items()}
    cases = [(f"{k} {label}", lambda k=k, v=v: gpu.denoise(**dict(good, **{k: v})), (k,))
             for k in good for label, v in _tensor_defects(good[k], anchor=k == "color")]
    host._check_all(cases)
    host._check_all([("workspace strided", lambda: gpu.denoise(good["color"], workspace=torch.zeros(1 << 17, dtype=torch.uint8, device="cuda")[::2]),
                      ("workspace",)),
                     ("workspace on the CPU", lambda: gpu.denoise(good["color"], workspace=torch.zeros(1 << 16, dtype=torch.uint8)), ("workspace",))])


def test_reproject(gpu):
    cams, planes, tables = host._reproject_args(gpu)
    dtypes = {k: v.dtype for k, v in tables.items()}
    planes = {k: _cuda(v) for k, v in planes.items()}
    tables = {k: torch.zeros((RECORDS, d.itemsize // 4), device="cuda") for k, d in dtypes.items()}
    good = dict(cams, **planes, **tables)
    cases = [(f"{k} {label}", lambda k=k, v=v: gpu.reproject(**dict(good, **{k: v})), (k,))
             for k in planes for label, v in _tensor_defects(planes[k], anchor=k == "color")]
    cases += [(f"{k} {label}", lambda k=k, v=v: gpu.reproject(**dict(good, **{k: v})), (k,))
              for k in tables for label, v in _table_defects(tables[k], dtypes[k], prev=k.startswith("prev_"))]
    host._check_all(cases)


@pytest.mark.parametrize("through", [False, True])
def test_aov(gpu, through):
    ds, f = host._scene(gpu), host._frame(gpu)
    table = gpu.AOV_THROUGH_OUTPUTS if through else gpu.AOV_OUTPUTS
    call = ds.render_aov_through if through else ds.render_aov
    good = {k: torch.zeros(RGB if ch == 3 else ONE, dtype=torch.float32 if dtype == np.float32 else torch.int32, device="cuda")
            for k, (ch, dtype) in table.items()}
    host._passes_the_binding(lambda: call(f, out=good))
    cases = []
    for k in good:
        for label, v in _tensor_defects(good[k], counted=True):
            names = (k, "out") if label == "a numpy array" else (k,)       # an array among tensors: `out` is what is wrong
            cases.append((f"{k} {label}", lambda k=k, v=v: call(f, out=dict(good, **{k: v})), names))
    host._check_all(cases)


@pytest.mark.parametrize("entry", ["render_variance", "render_adaptive"])
def test_frame_with_a_second_plane(gpu, entry):
    ds, f = host._scene(gpu), host._frame(gpu)
    second, dtype = ("variance_out", torch.float32) if entry == "render_variance" else ("spp_out", torch.int32)
    good = {"out": torch.zeros(RGB, device="cuda"), second: torch.zeros(ONE, dtype=dtype, device="cuda")}

    def call(**kw):
        method, args = (ds.render_variance, (f, 2)) if entry == "render_variance" else (ds.render_adaptive, (f, 2, 4, 0.1))
        return method(*args, **kw)
    host._passes_the_binding(lambda: call(**good))
    host._passes_the_binding(lambda: call(**{"out": good["out"], second: good[second].data_ptr()}))   # a tensor beside a pointer
    # (an array beside a tensor is refused as a pair, "out and ... must both be": tests/test_variance_host.py, test_adaptive_host.py)
    cases = [(f"{k} {label}", lambda k=k, v=v: call(**dict(good, **{k: v})), (k,))
             for k in good for label, v in _tensor_defects(good[k], anchor=k == "out", counted=True, among_arrays=False)]
    host._check_all(cases)


@pytest.mark.parametrize("entry", ["trace", "radiance"])
def test_ray_queries(gpu, entry):
    ds = host._scene(gpu)
    good = host._rays()
    if entry == "trace":
        good["tmax"] = np.full(len(good["times"]), 10.0, np.float32)
        call = ds.trace
    else:
        good["seeds"] = np.arange(len(good["times"]), dtype=np.int64)
        call = lambda **kw: ds.radiance(background=[0.0, 0.0, 0.0], gradient=False, **kw)   # noqa: E731
    good = {k: _cuda(v) for k, v in good.items()}
    host._passes_the_binding(lambda: call(**good))
    wide = torch.zeros((len(good["times"]), 6), device="cuda")
    host._passes_the_binding(lambda: call(**dict(good, origins=wide[:, :3], directions=wide[:, 3:])))   # copied, not refused
    cases = [(f"{k} {label}", lambda k=k, v=v: call(**dict(good, **{k: v})), (k,))
             for k in good for label, v in _tensor_defects(good[k], anchor=k == "origins", strided_ok=True)]
    host._check_all(cases)


@pytest.mark.parametrize("kind", ["spheres", "instances", "quads"])
def test_updates(gpu, kind):
    ds = host._scene(gpu)
    dtype = {"spheres": gpu.SPHERE_DTYPE, "instances": gpu.INSTANCE_DTYPE, "quads": gpu.QUAD_DTYPE}[kind]
    call = getattr(ds, "update_" + kind)
    good = torch.zeros((RECORDS, dtype.itemsize // 4), device="cuda")
    host._passes_the_binding(lambda: call(good))
    host._passes_the_binding(lambda: call(good.view(torch.int32), stream=torch.cuda.Stream()))
    call(good[:0])                                                                      # no record: nothing to do, no scene needed
    host._check_all([(label, lambda v=v: call(v), (kind,)) for label, v in _table_defects(good)])
    host._check_all([("indices of another length", lambda: call(good, indices=[0]), ("indices",))])
