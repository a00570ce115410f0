"""The owning device buffer that struct rt_scene, rt_progressive and call_memory hold (csrc/rt_owned.h) as a stand-alone program
under the address and undefined-behaviour sanitizers, over a counting fake allocator that can be told to fail: what grow
allocates and frees, a failed grow, moves, release and adopt, and that every allocation is freed exactly once, each against
values written out by hand in tests/owned_check.cpp.  No device, no HIP, nothing loaded into Python."""
import os
import subprocess


def test_owned_under_sanitizers(art, tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / "owned_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(art.PKG_DIR, "csrc"), "-o", str(exe), os.path.join(here, "owned_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "owned ok" and r.stderr == ""
