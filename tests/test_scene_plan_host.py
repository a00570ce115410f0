"""The decisions rt_scene_create makes before it uploads anything (csrc/rt_scene_plan.h) as a stand-alone program under the address
and undefined-behaviour sanitizers: the checks of a description and its class, the walk-array planner, the three regrouped
hierarchies (the sampled-ray one included, which no other test reaches without a device), the leaves-only array, the link encoding,
the tier data and the marks on quads, boxes and materials, each against values written out by hand in tests/scene_plan_check.cpp.
Built with the library's -ffp-contract=off.  No device, no HIP call, nothing loaded into Python."""
import os
import subprocess


def test_scene_plan_under_sanitizers(art, tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / "scene_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-I", os.path.join(art.PKG_DIR, "csrc"), "-o", str(exe),
                    os.path.join(here, "scene_plan_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "scene plan ok" and r.stderr == ""
