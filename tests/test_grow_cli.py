"""rayTracer --orbit ... --grow AMOUNT [--follow-quads]: the boxes of a resident scene change height frame by frame
(rt_scene_update_quads), and with --follow-quads the frames are accumulated over time, the history following the faces
(rt_reproject_quads)."""
import ctypes as C
import ctypes.util
import math
import os
import subprocess

import numpy as np
import pytest

import reproject_quads_expect as qx


def test_grow_and_follow_quads_refusals(art, tmp_path):
    """Status 2 and a message of its own before any device is touched: --grow without --orbit, with an AMOUNT that is not finite or
    not below 1 in magnitude, with --temporal, on a scene without a box; --follow-quads without --grow (with and without --orbit,
    with --temporal, with --spin ... --follow-instances).  The older refusals stay word for word."""
    exe = os.path.join(art.LIB_DIR, "rayTracer")
    base = [exe, "--nx", "16", "--ny", "8", "--ns", "2"]
    out = str(tmp_path / "x")
    orbit = ["--orbit", "2", "0", "--out", out]
    cases = [
        (["--scene", "cornell", "--grow", "0.2"], b"--grow needs --orbit\n"),
        (["--scene", "cornell"] + orbit + ["--grow", "1"], b"--grow AMOUNT: AMOUNT must be finite and |AMOUNT| < 1\n"),
        (["--scene", "cornell"] + orbit + ["--grow", "-1.5"], b"--grow AMOUNT: AMOUNT must be finite and |AMOUNT| < 1\n"),
        (["--scene", "cornell"] + orbit + ["--grow", "nan"], b"--grow AMOUNT: AMOUNT must be finite and |AMOUNT| < 1\n"),
        (["--scene", "cornell"] + orbit + ["--grow", "inf"], b"--grow AMOUNT: AMOUNT must be finite and |AMOUNT| < 1\n"),
        (["--scene", "cornell"] + orbit + ["--grow"], b"missing value for --grow\n"),
        (["--scene", "cornell"] + orbit + ["--grow", "0.2", "--temporal"],
         b"--grow cannot be combined with --temporal: the plain accumulation does not follow a box that changes size (--follow-quads does)\n"),
        (["--scene", "cornell"] + orbit + ["--grow", "0.2", "--temporal", "--follow-quads"], b"--grow cannot be combined with --temporal"),
        (["--scene", "book1"] + orbit + ["--grow", "0.2"], b"--grow: scene 'book1' has no box\n"),
        (["--scene", "quads"] + orbit + ["--grow", "0.2", "--follow-quads"], b"--grow: scene 'quads' has no box\n"),
        (["--scene", "cornell", "--follow-quads"], b"--follow-quads needs --orbit FRAMES DEGREES --grow AMOUNT"),
        (["--scene", "cornell"] + orbit + ["--follow-quads"], b"--follow-quads needs --orbit FRAMES DEGREES --grow AMOUNT"),
        (["--scene", "cornell"] + orbit + ["--temporal", "--follow-quads"], b"--follow-quads needs --orbit FRAMES DEGREES --grow AMOUNT"),
        (["--scene", "cornell"] + orbit + ["--spin", "10", "--follow-instances", "--follow-quads"], b"--follow-quads needs --orbit FRAMES DEGREES --grow AMOUNT"),
        # what was refused before is refused as before
        (["--scene", "cornell"] + orbit + ["--grow", "0.2", "--follow-instances"], b"--follow-instances needs --orbit FRAMES DEGREES --spin DEGREES"),
        (["--scene", "cornell"] + orbit + ["--grow", "0.2", "--spin", "10", "--temporal"], b"--spin cannot be combined with --temporal"),
        (["--scene", "cornell", "--grow", "0.2", "--gpus", "2"] + orbit, b"--orbit cannot be combined with --gpus > 1"),
    ]
    for extra, message in cases:
        r = subprocess.run(base + extra, capture_output=True, timeout=60)
        assert r.returncode == 2 and r.stdout == b"", (extra, r.returncode, r.stderr)
        assert (r.stderr == message) if message.endswith(b"\n") else (message in r.stderr), (extra, r.stderr)
    assert not list(tmp_path.iterdir())
    usage = open(os.path.join(art.PKG_DIR, "host", "main.cpp")).read().split("#include")[0]
    assert "[--grow AMOUNT [--follow-quads]]" in usage


def grown(art, base, k, frames, amount):
    """The executable's rule: every box of the description rebuilt with b'.y = (float)(a.y + (b.y - a.y)(1 + amount sin(2 pi k /
    frames))), in double, and the material of its first face."""
    rec = base.copy()
    boxes = [first for first in range(len(base) - 5) if _is_box(base[first:first + 6])]
    for first in boxes:
        a, b = qx.box_extent(base[first:first + 6])
        b = b.copy()
        b[1] = np.float32(float(a[1]) + (float(b[1]) - float(a[1])) * (1.0 + amount * math.sin(2.0 * math.pi * k / frames)))
        rec[first:first + 6] = art.box_records(a, b, int(base["mat"][first]))
    return rec, boxes


def _is_box(six):
    """Six records that are the faces of one axis-aligned box in make_box's order (the Cornell scenes hold no other six like it)."""
    codes = [int(np.flatnonzero(q["n"])[0]) if np.count_nonzero(q["n"]) == 1 else -1 for q in six]
    return codes == [2, 0, 2, 0, 1, 1] and len(set(six["mat"].tolist())) == 1


@pytest.mark.gpu
def test_grow_with_follow_quads_equals_the_python_sequence(gpu, tmp_path):
    """Three frames of the Cornell box at 32 x 32 under a still camera, its two blocks growing and shrinking by a fifth, accumulated:
    byte for byte the images of TemporalAccumulator(follow_quads=True) pushed with the records the executable's rule gives, with
    the gamma applied as the executable applies it (libm's powf).  Without the flag the frames are other images, and the blocks
    keep a history: some pixel that shows a face of a block has a history longer than one frame."""
    exe = os.path.join(gpu.LIB_DIR, "rayTracer")
    nx, ny, ns, frames, amount = 32, 32, 4, 3, 0.2
    base = [exe, "--scene", "cornell", "--nx", str(nx), "--ny", str(ny), "--ns", str(ns)]
    r = subprocess.run(base + ["--orbit", str(frames), "0", "--grow", str(amount), "--follow-quads", "--out", str(tmp_path / "f")],
                       capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    got = [(tmp_path / f"f_{k:03d}.ppm").read_bytes() for k in range(frames)]
    r = subprocess.run(base + ["--orbit", str(frames), "0", "--grow", str(amount), "--out", str(tmp_path / "s")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert all(got[k] != (tmp_path / f"s_{k:03d}.ppm").read_bytes() for k in range(1, frames))

    hs = gpu.HostScene("cornell", nx, ny)
    base_records = hs.quads().copy()
    powf = C.CDLL(ctypes.util.find_library("m") or "libm.so.6").powf
    powf.argtypes, powf.restype = [C.c_float, C.c_float], C.c_float
    exponent = float(np.float32(1.0) / np.float32(hs.gamma))
    ds = gpu.DeviceScene(hs)
    try:
        acc = gpu.TemporalAccumulator(ds, hs.frame(nx=nx, ny=ny, ns=ns, seed_base=1984), follow_quads=True)
        for k in range(frames):
            rec, boxes = grown(gpu, base_records, k, frames, amount)
            assert boxes == [3, 10]
            out = acc.push(hs.desc.camera, quads=rec)
            assert not qx.quad_records_differ(ds.quads(), rec).any()
            if hs.gamma != 1.0:
                out = np.array([powf(float(c), exponent) for c in out.reshape(-1)], np.float32).reshape(ny, nx, 3)
            path = str(tmp_path / f"py_{k}.ppm")
            gpu.write_ppm(path, out, hs.ppm_double_scale)
            assert open(path, "rb").read() == got[k], f"frame {k}"
        faces = [q for first in boxes for q in range(first, first + 6)]
        on_block = qx.shows_moved(acc._prev["prim"], acc._prev["inst"], len(base_records), len(hs.instances()), faces)
        assert on_block.any() and (acc.length[on_block] > 1).any()
    finally:
        ds.close()
        hs.close()
