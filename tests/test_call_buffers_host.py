"""The buffer table that rt_render_aov*, rt_denoise*, rt_upscale and rt_reproject* share (csrc/rt_call_buffers.h) as a
stand-alone program under the address and undefined-behaviour sanitizers: the overlap test, the size of the staging allocation
and the order in which its pieces are taken, each against values written out by hand in tests/call_buffers_check.cpp.  No
device, no HIP, nothing loaded into Python."""
import os
import subprocess


def test_call_buffers_under_sanitizers(art, tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / "call_buffers_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(art.PKG_DIR, "csrc"), "-o", str(exe), os.path.join(here, "call_buffers_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "call buffers ok" and r.stderr == ""
