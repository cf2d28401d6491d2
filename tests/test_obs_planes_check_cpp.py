"""The host's description of the planes of the OBS video formats and the routing of lvk_hip_scale_obs (livevisionkit_amd/csrc/obs_planes.hpp, DESIGN.md
section 30) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: the rows and spans of every format against a brute-force byte map, the
parity rules, the 4:2:0 plane sets and the route table.  tests/cpp/obs_planes_check.cpp, a stand-alone program, g++ only: the header needs no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_obs_planes_rules_against_a_byte_map_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "obs_planes_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "livevisionkit_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "obs_planes_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "obs planes ok" in out.stdout, out.stdout + out.stderr
