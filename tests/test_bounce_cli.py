"""rayTracer --orbit ... --bounce HEIGHT: the small spheres of a scene moved before every frame through rt_scene_update_spheres, and
with --temporal an accumulation that follows them (rt_reproject_moving)."""
import ctypes as C
import ctypes.util
import math
import os
import subprocess

import numpy as np
import pytest


def test_bounce_needs_orbit_and_a_scene_without_instances(art, tmp_path):
    """Status 2 and a message before any device is touched: --bounce without --orbit, a negative or non-finite HEIGHT, and a
    scene with instances (a sphere under an instance cannot be updated)."""
    exe = os.path.join(art.LIB_DIR, "rayTracer")
    base = [exe, "--nx", "16", "--ny", "8", "--ns", "2"]
    out = str(tmp_path / "x")
    for extra in (["--bounce", "0.2"], ["--bounce", "0.2", "--temporal"], ["--orbit", "2", "0", "--out", out, "--bounce", "-0.5"],
                  ["--orbit", "2", "0", "--out", out, "--bounce", "nan"], ["--orbit", "2", "0", "--out", out, "--bounce", "inf"],
                  ["--orbit", "2", "0", "--out", out, "--bounce"],
                  ["--scene", "instanced", "--orbit", "2", "0", "--out", out, "--bounce", "0.2"],
                  ["--scene", "cornell", "--orbit", "2", "10", "--out", out, "--bounce", "0.2", "--temporal"]):
        r = subprocess.run(base + extra, capture_output=True, timeout=60)
        assert r.returncode == 2 and r.stderr and r.stdout == b"", (extra, r.returncode, r.stderr)
        assert b"--bounce" in r.stderr or b"--orbit" in r.stderr, (extra, r.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.gpu
def test_bounce_with_temporal_equals_the_python_sequence(gpu, tmp_path):
    """Three frames of book1 at 32 x 16 under a still camera, the small spheres bouncing by up to 0.2, accumulated: byte for
    byte the images of TemporalAccumulator(follow_spheres=True) pushed with the records the executable's rule gives, with the
    gamma applied as the executable applies it (libm's powf).  Without --bounce the later frames are other images."""
    exe = os.path.join(gpu.LIB_DIR, "rayTracer")
    nx, ny, ns, frames, height = 32, 16, 4, 3, 0.2
    base = [exe, "--scene", "book1", "--nx", str(nx), "--ny", str(ny), "--ns", str(ns)]
    r = subprocess.run(base + ["--orbit", str(frames), "0", "--out", str(tmp_path / "b"), "--bounce", str(height), "--temporal"],
                       capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    got = [(tmp_path / f"b_{k:03d}.ppm").read_bytes() for k in range(frames)]
    r = subprocess.run(base + ["--orbit", str(frames), "0", "--out", str(tmp_path / "s"), "--temporal"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    still = [(tmp_path / f"s_{k:03d}.ppm").read_bytes() for k in range(frames)]
    assert got[0] != still[0] and got[1] != still[1]          # (the rule lifts every small sphere but sphere 0 in frame 0 already)

    hs = gpu.HostScene("book1", nx, ny)
    base_records = hs.spheres()
    small = np.flatnonzero((base_records["radius"] > 0) & (base_records["radius"] < 0.5))
    assert len(small) > 10 and len(hs.instances()) == 0
    powf = C.CDLL(ctypes.util.find_library("m") or "libm.so.6").powf
    powf.argtypes, powf.restype = [C.c_float, C.c_float], C.c_float
    exponent = float(np.float32(1.0) / np.float32(hs.gamma))
    ds = gpu.DeviceScene(hs)
    try:
        acc = gpu.TemporalAccumulator(ds, hs.frame(nx=nx, ny=ny, ns=ns, seed_base=1984), follow_spheres=True)
        for k in range(frames):
            rec = base_records.copy()
            for i in small:
                rec["c0"][i, 1] = np.float32(float(base_records["c0"][i, 1]) + height * abs(math.sin(math.pi * (k / frames + 0.61803398875 * int(i)))))
            out = acc.push(hs.desc.camera, spheres=rec)
            assert ds.spheres().tobytes() == rec.tobytes()
            if hs.gamma != 1.0:
                out = np.array([powf(float(c), exponent) for c in out.reshape(-1)], np.float32).reshape(ny, nx, 3)
            path = str(tmp_path / f"py_{k}.ppm")
            gpu.write_ppm(path, out, hs.ppm_double_scale)
            assert open(path, "rb").read() == got[k], f"frame {k}"
        assert (acc.length > 1).any()
    finally:
        ds.close()
        hs.close()
