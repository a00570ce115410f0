"""rt_render_variance / DeviceScene.render_variance on the GPU: the frame, every pixel's variance (as bits), the ray and sample
totals equal what the CPU oracle predicts (tests/variance_expect.py); the identity with rt_render; a row-partitioned share;
device outputs; no clobbered scene state; the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_expect as ax
import variance_expect as vx

pytestmark = pytest.mark.gpu

NX, NY = 32, 24
# every scene with one (ns, B): batches of two samples, of three, and B = n (batches of one)
CASES = [("bouncing", 8, 4), ("cornell", 6, 2), ("cornell_smoke", 16, 16), ("final", 8, 4), ("instanced", 6, 2), ("crowd_4097", 16, 16),
         ("degenerate", 8, 4)]


@pytest.fixture(scope="module")
def scenes(gpu, orc):
    cache = {}

    def get(name, nx=NX, ny=NY):
        key = (name, nx, ny)
        if key not in cache:
            img, iw, ih = gpu.default_texture(name)
            hs = gpu.HostScene(name, nx, ny, img, iw, ih)
            ex = ax.Expectation(orc.OracleScene(name, nx, ny, img, iw, ih))
            cache[key] = (hs, gpu.DeviceScene(hs), ex)
        return cache[key]
    yield get
    for _, ds, _ in cache.values():
        ds.close()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


@pytest.mark.parametrize("name,ns,B", CASES)
def test_frame_and_variance_match_oracle(scenes, name, ns, B):
    hs, ds, ex = scenes(name)
    fb, var, st = ds.render_variance(hs.frame(ns=ns), B)
    efb, evar = vx.render_variance(ex, ns, B, hs.gamma)
    _same(fb, efb, "fb")
    _same(var, evar, "variance")
    assert (evar > 0).any()
    assert st.rays == int(ex.rays(ns).sum()) and st.samples == NX * NY * ns
    assert st.local_rows == NY and st.reserved == B
    # the frame, rays and samples of rt_render at the same ns
    ref, rst = ds.render(hs.frame(ns=ns))
    _same(fb, ref, "fb against render")
    assert st.rays == rst.rays and st.samples == rst.samples


def test_variance_is_linear_whatever_the_gamma(scenes):
    hs, ds, ex = scenes("bouncing")
    fb1, var1, _ = ds.render_variance(hs.frame(ns=8, gamma=1.0), 4)
    fb2, var2, _ = ds.render_variance(hs.frame(ns=8, gamma=2.2), 4)
    _same(var1, var2, "variance")
    _same(fb2, ex.frame(8, 2.2), "fb at gamma 2.2")
    assert not np.array_equal(_bits(fb1), _bits(fb2))


@pytest.mark.parametrize("name,ns,B", [("bouncing", 8, 4), ("cornell", 6, 2)])
def test_row_partition(gpu, scenes, name, ns, B):
    """4-row tiles dealt to a world of 3: each share equals the matching rows of the whole frame."""
    hs, ds, ex = scenes(name)
    whole, wvar, wst = ds.render_variance(hs.frame(ns=ns), B)
    rays = samples = 0
    for rank in range(3):
        f = hs.frame(ns=ns, tile_rows=4, tile_first=rank, tile_stride=3)
        rows = gpu.local_rows_to_global(f)
        fb, var, st = ds.render_variance(f, B)
        assert fb.shape == (len(rows), NX, 3) and var.shape == (len(rows), NX) and st.local_rows == len(rows)
        _same(fb, whole[rows], f"fb of rank {rank}")
        _same(var, wvar[rows], f"variance of rank {rank}")
        rays += st.rays
        samples += st.samples
    assert rays == wst.rays and samples == wst.samples


def test_device_outputs(gpu, scenes):
    import torch
    hs, ds, ex = scenes("cornell")
    fb, var, st = ds.render_variance(hs.frame(ns=6), 2)
    out = torch.full((NY, NX, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    vard = torch.full((NY, NX), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    r_fb, r_var, st2 = ds.render_variance(hs.frame(ns=6), 2, out=out, variance_out=vard, stream=side)
    assert r_fb is out and r_var is vard
    _same(out.cpu().numpy(), fb, "device fb")
    _same(vard.cpu().numpy(), var, "device variance")
    assert st2.rays == st.rays and st2.samples == st.samples
    with pytest.raises(ValueError):
        ds.render_variance(hs.frame(ns=6), 2, out=out, variance_out=np.zeros((NY, NX), np.float32))


def test_render_and_adaptive_unchanged_after_a_variance_frame(scenes):
    hs, ds, ex = scenes("final")
    before_fb, before_st = ds.render(hs.frame(ns=40))
    before_ad = ds.render_adaptive(hs.frame(ns=1), 4, 32, 0.05, 0.01)
    ds.render_variance(hs.frame(ns=16), 16)
    after_fb, after_st = ds.render(hs.frame(ns=40))
    after_ad = ds.render_adaptive(hs.frame(ns=1), 4, 32, 0.05, 0.01)
    _same(before_fb, after_fb, "render")
    assert before_st.rays == after_st.rays
    _same(before_ad[0], after_ad[0], "adaptive fb")
    assert np.array_equal(before_ad[1], after_ad[1]) and before_ad[2].rays == after_ad[2].rays and before_ad[2].samples == after_ad[2].samples


def test_cli_prints_the_python_pipeline(gpu, scenes, tmp_path):
    """rayTracer --denoise --denoise-variance: render_denoised(variance=True) of the same frame, the frame's gamma applied
    afterwards as the program applies it (powf(c, 1 / gamma), the C library's)."""
    nx, ny, ns = 40, 30, 8
    hs, ds, _ = scenes("bouncing", nx, ny)
    exe = os.path.join(gpu.PKG_DIR, "lib", "rayTracer")
    r = subprocess.run([exe, "--scene", "bouncing", "--nx", str(nx), "--ny", str(ny), "--ns", str(ns), "--denoise", "--denoise-variance"],
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    res = ds.render_denoised(hs.frame(ns=ns), variance=True)          # batches: 8, the largest divisor of 8 up to 16
    plain = ds.render_denoised(hs.frame(ns=ns))
    assert not np.array_equal(res["color"], plain["color"])
    _same(res["noisy"], plain["noisy"], "noisy")
    img = res["color"].copy()
    if hs.gamma != 1.0:
        libm = C.CDLL("libm.so.6")
        libm.powf.restype, libm.powf.argtypes = C.c_float, [C.c_float, C.c_float]
        e = float(np.float32(1.0) / np.float32(hs.gamma))
        img = np.array([libm.powf(float(c), e) for c in img.ravel()], np.float32).reshape(img.shape)
    path = tmp_path / "py.ppm"
    gpu.write_ppm(str(path), img, hs.ppm_double_scale)
    assert r.stdout == path.read_bytes()
