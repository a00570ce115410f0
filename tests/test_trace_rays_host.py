"""rt_trace_rays without a device: the export, the batch layout against the header, the argument checks that run before
any HIP call, and the two trace options."""
import ctypes as C
import os
import subprocess

import pytest

RT_ERR_INVALID = 1
FAKE = 0x1000   # never dereferenced: every check below fails before a pointer is looked at


def test_trace_rays_is_exported(art):
    assert "rt_trace_rays" in art.RT_ABI_SYMBOLS
    assert hasattr(art.rt_lib(), "rt_trace_rays")


def test_ray_batch_layout_matches_header(art, tmp_path):
    """sizeof and every field offset of rt_ray_batch as a C compiler lays out include/rt_abi.h."""
    fields = [f for f, _ in art.RtRayBatch._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rt_abi.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(rt_ray_batch));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof(rt_ray_batch, {f}));\n" for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(art.REPO_ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(art.RtRayBatch) == 112
    assert got[1:] == [getattr(art.RtRayBatch, f).offset for f in fields]


def _batch(art, **kw):
    b = art.RtRayBatch()
    b.n, b.origins, b.directions, b.tmin, b.mode = 4, FAKE, FAKE, 0.001, art.RT_TRACE_CLOSEST
    b.t_out, b.prim_out = FAKE, FAKE
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _call(art, scene, batch):
    L = art.rt_lib()
    st = L.rt_trace_rays(scene, None if batch is None else C.byref(batch), None, 1)
    return st, L.rt_last_error_detail().decode()


def test_argument_checks_name_what_failed(art):
    """Every case passes a null scene: the text shows that the batch check fired first, with no device touched."""
    cases = {
        "null batch": None,
        "n < 0": _batch(art, n=-1),
        "NaN tmin": _batch(art, tmin=float("nan")),
        "infinite tmin": _batch(art, tmin=float("inf")),
        "unknown mode": _batch(art, mode=7),
        "ANY with t_out": _batch(art, mode=art.RT_TRACE_ANY, prim_out=None, hit_out=FAKE),
        "ANY without hit_out": _batch(art, mode=art.RT_TRACE_ANY, t_out=None, prim_out=None),
        "CLOSEST without prim_out": _batch(art, prim_out=None),
        "CLOSEST with hit_out": _batch(art, hit_out=FAKE),
        "null origins": _batch(art, origins=None),
    }
    texts = {}
    for name, b in cases.items():
        st, text = _call(art, None, b)
        assert st == RT_ERR_INVALID, name
        assert "null scene" not in text, (name, text)
        texts[name] = text
    st, text = _call(art, None, _batch(art))
    assert st == RT_ERR_INVALID and "null scene" in text
    texts["null scene"] = text
    must_differ = ["null batch", "n < 0", "NaN tmin", "unknown mode", "ANY with t_out", "null scene"]
    assert len({texts[k] for k in must_differ}) == len(must_differ), texts
    assert texts["NaN tmin"] == texts["infinite tmin"]


@pytest.mark.parametrize("key,good,bad", [("trace_lds", [-1, 0, 1, 2], [-2, 3]), ("trace_tree", [0, 1], [-1, 2])])
def test_trace_options(art, key, good, bad):
    L = art.rt_lib()
    try:
        for v in good:
            assert L.rt_set_option(key.encode(), v) == 0, (key, v)
        for v in bad:
            assert L.rt_set_option(key.encode(), v) == RT_ERR_INVALID, (key, v)
            assert key in L.rt_last_error_detail().decode()
    finally:
        assert L.rt_reset_options() == 0


def test_reset_restores_trace_defaults(art):
    """The options have no getter; without a device what can be seen is that the reset succeeds after each key was moved
    off its default and that the defaults are accepted again (the GPU tests run every value and reset after each)."""
    L = art.rt_lib()
    assert L.rt_set_option(b"trace_lds", 0) == 0 and L.rt_set_option(b"trace_tree", 0) == 0
    assert L.rt_reset_options() == 0
    assert L.rt_set_option(b"trace_lds", -1) == 0 and L.rt_set_option(b"trace_tree", 1) == 0
    assert L.rt_reset_options() == 0


def test_any_hit_with_record_is_rejected_before_any_device_work(art):
    """DeviceScene.trace(any_hit=True, record=True): the C entry point takes no record outputs in ANY mode, so the binding
    raises ValueError at once instead of dropping `record`."""
    import numpy as np
    ds = art.DeviceScene.__new__(art.DeviceScene)   # no device scene needed: the check comes first
    ds.device, ds._p = 0, C.c_void_p()
    o = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="record"):
        ds.trace(o, o, any_hit=True, record=True)
