"""rayTracer --upscale F on the GPU: the PPM is, byte for byte, what DeviceScene.render_upscaled and the host's gamma give --
with and without --denoise -- and the flag's refusals exit with 2."""
import ctypes as C
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCENE, NX, NY, NS = "bouncing", 32, 24, 4


def _host_gamma(img, gamma):
    """powf(c, 1.0f / gamma) per channel with the C library's powf, as host/main.cpp applies it."""
    if gamma == 1.0:
        return img
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.powf.restype, libm.powf.argtypes = C.c_float, [C.c_float, C.c_float]
    e = float(np.float32(1.0) / np.float32(gamma))
    return np.array([libm.powf(float(c), e) for c in img.reshape(-1)], np.float32).reshape(img.shape)


@pytest.mark.parametrize("denoise", [False, True])
def test_cli_writes_render_upscaled(gpu, tmp_path, denoise):
    exe = os.path.join(gpu.LIB_DIR, "rayTracer")
    cmd = [exe, "--scene", SCENE, "--nx", str(NX), "--ny", str(NY), "--ns", str(NS), "--p6", "--upscale", "2"] + (["--denoise"] if denoise else [])
    r = subprocess.run(cmd, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    hs = gpu.HostScene(SCENE, NX, NY)
    ds = gpu.DeviceScene(hs)
    try:
        got = ds.render_upscaled(hs.frame(ns=NS), 2, denoise=denoise)
    finally:
        ds.close()
    assert got["color"].shape == (NY, NX, 3)
    path = tmp_path / "py.ppm"
    gpu.write_ppm(str(path), _host_gamma(got["color"], hs.gamma), hs.ppm_double_scale, binary=True)
    assert path.read_bytes() == r.stdout
    plain = subprocess.run(cmd[:cmd.index("--upscale")], capture_output=True, timeout=120)      # the frame without the flag has the same size
    assert plain.returncode == 0 and len(plain.stdout) == len(r.stdout) and plain.stdout != r.stdout


def test_cli_refusals_exit_2(gpu):
    exe = os.path.join(gpu.LIB_DIR, "rayTracer")
    base = [exe, "--scene", SCENE, "--nx", str(NX), "--ny", str(NY), "--ns", "2", "--upscale"]
    for extra in (["2", "--gpus", "2"], ["2", "--progressive", "2"], ["2", "--adaptive", "0.1"], ["2", "--orbit", "2", "10", "--out", "x"],
                  ["2", "--aov", "x"], ["2", "--aov-through", "x"], ["2", "--denoise", "--denoise-variance"], ["2", "--denoise", "--denoise-through"],
                  ["5"], ["3", "--ny", "33"], ["1"], ["9"]):
        r = subprocess.run(base + extra, capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--upscale" in r.stderr and r.stdout == b"", (extra, r.returncode, r.stderr)
