"""rayTracer --orbit ... --spin DEGREES: the rotated instances of a scene turned before every frame through
rt_scene_update_instances."""
import math
import os
import subprocess

import numpy as np
import pytest


def test_spin_needs_orbit_and_a_rotated_instance(art, tmp_path):
    """Status 2 and a message before any device is touched: --spin without --orbit, a non-finite or missing DEGREES, a scene
    without a rotated instance, and --spin with --temporal (the reprojection does not follow a moved instance)."""
    exe = os.path.join(art.LIB_DIR, "rayTracer")
    base = [exe, "--nx", "16", "--ny", "8", "--ns", "2"]
    out = str(tmp_path / "x")
    for extra in (["--scene", "cornell", "--spin", "10"],
                  ["--scene", "cornell", "--orbit", "2", "0", "--out", out, "--spin", "nan"],
                  ["--scene", "cornell", "--orbit", "2", "0", "--out", out, "--spin", "inf"],
                  ["--scene", "cornell", "--orbit", "2", "0", "--out", out, "--spin"],
                  ["--scene", "book1", "--orbit", "2", "0", "--out", out, "--spin", "10"],
                  ["--orbit", "2", "0", "--out", out, "--spin", "10"],
                  ["--scene", "cornell", "--orbit", "2", "0", "--out", out, "--spin", "10", "--temporal"]):
        r = subprocess.run(base + extra, capture_output=True, timeout=60)
        assert r.returncode == 2 and r.stderr and r.stdout == b"", (extra, r.returncode, r.stderr)
        assert b"--spin" in r.stderr, (extra, r.stderr)
    # --bounce keeps its refusal on scenes with instances
    r = subprocess.run(base + ["--scene", "cornell", "--orbit", "2", "0", "--out", out, "--bounce", "0.2"], capture_output=True, timeout=60)
    assert r.returncode == 2 and b"--bounce" in r.stderr
    assert not list(tmp_path.iterdir())


@pytest.mark.gpu
def test_spin_equals_the_python_sequence(gpu, tmp_path):
    """Three frames of the Cornell box at 32 x 32 under a still camera, its two blocks turning by 10 degrees a frame: byte for
    byte the images of DeviceScene.update_instances with the records the executable's rule gives, then render and write_ppm.
    Without --spin frame 1 is another image."""
    exe = os.path.join(gpu.LIB_DIR, "rayTracer")
    nx, ny, ns, frames, degrees = 32, 32, 4, 3, 10.0
    base = [exe, "--scene", "cornell", "--nx", str(nx), "--ny", str(ny), "--ns", str(ns)]
    r = subprocess.run(base + ["--orbit", str(frames), "0", "--out", str(tmp_path / "t"), "--spin", str(degrees)], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    got = [(tmp_path / f"t_{k:03d}.ppm").read_bytes() for k in range(frames)]
    r = subprocess.run(base + ["--orbit", str(frames), "0", "--out", str(tmp_path / "s")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    still = [(tmp_path / f"s_{k:03d}.ppm").read_bytes() for k in range(frames)]
    assert got[1] != still[1] and got[2] != still[2]

    hs = gpu.HostScene("cornell", nx, ny)
    base_records = hs.instances()
    rotated = np.flatnonzero(base_records["flags"] & gpu.RT_INST_ROTATE_Y)
    assert len(rotated) == 2
    ds = gpu.DeviceScene(hs)
    try:
        frame = hs.frame(nx=nx, ny=ny, ns=ns, seed_base=1984)
        for k in range(frames):
            rec = base_records.copy()
            for i in rotated:
                a = math.atan2(float(base_records["sin_t"][i]), float(base_records["cos_t"][i])) + k * degrees * math.pi / 180.0
                rec["sin_t"][i], rec["cos_t"][i] = np.float32(math.sin(a)), np.float32(math.cos(a))
            ds.update_instances(rec)
            assert ds.instances().tobytes() == rec.tobytes()
            fb, _ = ds.render(frame)
            path = str(tmp_path / f"py_{k}.ppm")
            gpu.write_ppm(path, fb, hs.ppm_double_scale)
            assert open(path, "rb").read() == got[k], f"frame {k}"
    finally:
        ds.close()
        hs.close()
