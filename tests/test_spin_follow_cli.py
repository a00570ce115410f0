"""rayTracer --orbit ... --spin DEGREES --follow-instances: the frames accumulated over time, the history following the instances
that --spin turns (rt_reproject_instances)."""
import ctypes as C
import ctypes.util
import math
import os
import subprocess

import numpy as np
import pytest


def test_follow_instances_needs_spin(art, tmp_path):
    """Status 2 and a message of its own before any device is touched: --follow-instances without --spin (with and without --orbit,
    with --temporal, with --bounce); with --spin and --temporal together the older refusal stays."""
    exe = os.path.join(art.LIB_DIR, "rayTracer")
    base = [exe, "--nx", "16", "--ny", "8", "--ns", "2"]
    out = str(tmp_path / "x")
    for extra in (["--scene", "cornell", "--follow-instances"],
                  ["--scene", "cornell", "--orbit", "2", "0", "--out", out, "--follow-instances"],
                  ["--scene", "cornell", "--orbit", "2", "0", "--out", out, "--temporal", "--follow-instances"],
                  ["--scene", "book1", "--orbit", "2", "0", "--out", out, "--bounce", "0.2", "--follow-instances"]):
        r = subprocess.run(base + extra, capture_output=True, timeout=60)
        assert r.returncode == 2 and r.stderr and r.stdout == b"", (extra, r.returncode, r.stderr)
        assert b"--follow-instances needs" in r.stderr and b"--spin" in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + ["--scene", "cornell", "--orbit", "2", "0", "--out", out, "--spin", "10", "--temporal", "--follow-instances"],
                       capture_output=True, timeout=60)
    assert r.returncode == 2 and b"--spin cannot be combined with --temporal" in r.stderr
    r = subprocess.run(base + ["--scene", "book1", "--orbit", "2", "0", "--out", out, "--spin", "10", "--follow-instances"], capture_output=True, timeout=60)
    assert r.returncode == 2 and b"no rotated instance" in r.stderr
    assert not list(tmp_path.iterdir())


@pytest.mark.gpu
def test_spin_with_follow_instances_equals_the_python_sequence(gpu, tmp_path):
    """Three frames of the Cornell box at 32 x 32 under a still camera, its two blocks turning by 10 degrees a frame, accumulated:
    byte for byte the images of TemporalAccumulator(follow_instances=True) pushed with the records the executable's rule gives,
    with the gamma applied as the executable applies it (libm's powf).  Without the flag the frames are other images, and the
    blocks keep a history: some pixel that shows a block has a history longer than one frame."""
    exe = os.path.join(gpu.LIB_DIR, "rayTracer")
    nx, ny, ns, frames, degrees = 32, 32, 4, 3, 10.0
    base = [exe, "--scene", "cornell", "--nx", str(nx), "--ny", str(ny), "--ns", str(ns)]
    r = subprocess.run(base + ["--orbit", str(frames), "0", "--spin", str(degrees), "--follow-instances", "--out", str(tmp_path / "f")],
                       capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    got = [(tmp_path / f"f_{k:03d}.ppm").read_bytes() for k in range(frames)]
    r = subprocess.run(base + ["--orbit", str(frames), "0", "--spin", str(degrees), "--out", str(tmp_path / "s")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert all(got[k] != (tmp_path / f"s_{k:03d}.ppm").read_bytes() for k in range(1, frames))

    hs = gpu.HostScene("cornell", nx, ny)
    base_records = hs.instances().copy()
    rotated = np.flatnonzero(base_records["flags"] & gpu.RT_INST_ROTATE_Y)
    assert len(rotated) == 2
    powf = C.CDLL(ctypes.util.find_library("m") or "libm.so.6").powf
    powf.argtypes, powf.restype = [C.c_float, C.c_float], C.c_float
    exponent = float(np.float32(1.0) / np.float32(hs.gamma))
    ds = gpu.DeviceScene(hs)
    try:
        acc = gpu.TemporalAccumulator(ds, hs.frame(nx=nx, ny=ny, ns=ns, seed_base=1984), follow_instances=True)
        for k in range(frames):
            rec = base_records.copy()
            for i in rotated:
                a = math.atan2(float(base_records["sin_t"][i]), float(base_records["cos_t"][i])) + k * degrees * math.pi / 180.0
                rec["sin_t"][i], rec["cos_t"][i] = np.float32(math.sin(a)), np.float32(math.cos(a))
            out = acc.push(hs.desc.camera, instances=rec)
            assert ds.instances().tobytes() == rec.tobytes()
            if hs.gamma != 1.0:
                out = np.array([powf(float(c), exponent) for c in out.reshape(-1)], np.float32).reshape(ny, nx, 3)
            path = str(tmp_path / f"py_{k}.ppm")
            gpu.write_ppm(path, out, hs.ppm_double_scale)
            assert open(path, "rb").read() == got[k], f"frame {k}"
        on_block = np.isin(acc._prev["inst"], rotated)
        assert on_block.any() and (acc.length[on_block] > 1).any()
    finally:
        ds.close()
        hs.close()
