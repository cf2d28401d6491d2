"""Builds a C++ driver of the facade (tests/cpp/*.cpp) against include/ and liblvk_hip.so: the helper of tests/test_*_facade.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_facade(tmp_path, src, extra_flags=()):
    """Compiles `src` into tmp_path and returns the executable's path."""
    import torch
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib")
    exe = str(tmp_path / os.path.splitext(os.path.basename(src))[0])
    subprocess.check_call(["g++", "-std=c++20", "-Wall", "-O1", *extra_flags, "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + os.path.join(ROOT, "livevisionkit_amd"), "-llvk_hip", "-L" + tlib, "-l:libamdhip64.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "livevisionkit_amd"), "-Wl,-rpath," + tlib])
    return exe
