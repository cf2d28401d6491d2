"""The routing of lvk_hip_fsr_obs (fsr_route of livevisionkit_amd/csrc/obs_planes.hpp) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: the route of all sixteen formats and of numbers that are none, on the staged and on the direct path.
tests/cpp/fsr_route_check.cpp, a stand-alone program, g++ only: the header needs no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fsr_route_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fsr_route_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "livevisionkit_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "fsr_route_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fsr route ok" in out.stdout, out.stdout + out.stderr
