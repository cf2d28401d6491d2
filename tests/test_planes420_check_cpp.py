"""The host's rules about the planes of an I420 / NV12 frame (livevisionkit_amd/csrc/planes420.hpp) on the CPU: "well formed"
on hand-written cases, "the outputs are pairwise disjoint" and "the inputs are clear of the outputs" against a brute-force byte map of plane sets in a
256-byte arena.  tests/cpp/planes420_check.cpp, g++ only: the header needs no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planes420_rules_against_a_byte_map(tmp_path):
    exe = str(tmp_path / "planes420_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "livevisionkit_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "planes420_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "planes420 ok" in out.stdout, out.stdout + out.stderr
