"""The decisions rt_render, rt_render_window, rt_render_adaptive and rt_render_variance make before they enqueue anything
(csrc/rt_frame_plan.h) as a stand-alone program under the address and undefined-behaviour sanitizers: the main launch, the tier
room, the tier sizes, whether a frame is ranked, the hand-off and the parts of a frame, each against values written out by hand in
tests/frame_plan_check.cpp.  A wrong decision renders the right frame, only slower, so no frame comparison sees it.  No device,
no HIP call, nothing loaded into Python."""
import os
import subprocess


def test_frame_plan_under_sanitizers(art, tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / "frame_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I", os.path.join(art.PKG_DIR, "csrc"), "-o", str(exe),
                    os.path.join(here, "frame_plan_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "frame plan ok" and r.stderr == ""
