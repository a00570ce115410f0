"""rayTracer --orbit on the GPU: a turntable of one device scene through rt_scene_set_camera, optionally accumulated over time."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_orbit_writes_one_image_per_frame(gpu, tmp_path):
    """Frame 0 is the scene's own camera built again from its arguments: the image the plain program prints.  Later frames are
    other views; with --temporal every frame is written too and the first differs from the plain one only by how the gamma is
    applied."""
    exe = os.path.join(gpu.LIB_DIR, "rayTracer")
    base = [exe, "--scene", "book1", "--nx", "32", "--ny", "16", "--ns", "4"]
    plain = subprocess.run(base, capture_output=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout.startswith(b"P3"), plain.stderr
    r = subprocess.run(base + ["--orbit", "3", "45", "--out", str(tmp_path / "turn")], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    frames = [(tmp_path / f"turn_{k:03d}.ppm").read_bytes() for k in range(3)]
    assert frames[0] == plain.stdout
    assert frames[1] != frames[0] and frames[2] != frames[1] and all(f.startswith(b"P3") for f in frames)
    assert not (tmp_path / "turn_003.ppm").exists()
    r = subprocess.run(base + ["--orbit", "3", "6", "--out", str(tmp_path / "acc"), "--temporal"], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    acc = [(tmp_path / f"acc_{k:03d}.ppm").read_bytes().split() for k in range(3)]
    assert all(a[:4] == [b"P3", b"32", b"16", b"255"] and len(a) == 4 + 32 * 16 * 3 for a in acc)
    first = plain.stdout.split()
    assert max(abs(int(x) - int(y)) for x, y in zip(acc[0][4:], first[4:])) <= 1          # powf on the host against the kernel's gamma
    assert acc[1] != acc[0]
