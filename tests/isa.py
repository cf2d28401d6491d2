"""The gfx950 assembly hipcc emits for one unit of livevisionkit_amd/csrc with the Makefile's own flags (no GPU needed), and each kernel's
scratch size and VGPR count read from it: the helper of the ISA tests (tests/test_*_isa.py, tests/test_isa_budget.py)."""
import functools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livevisionkit_amd", "csrc")


def makefile_flags(unit):
    """csrc/Makefile's HIPFLAGS for gfx950 with absolute include paths, plus MESH_FLAGS for mesh.hip."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS = (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    includes = {"-I../../include": "-I" + os.path.join(ROOT, "include"), "-I.": "-I" + CSRC}
    flags = [includes.get(f, f) for f in flags]
    if unit == "mesh":
        flags += re.search(r"^MESH_FLAGS \?= (.*)$", text, re.M).group(1).split()
    return flags


@functools.lru_cache(maxsize=None)
def assemble(unit):
    """(assembly, {kernel: (scratch bytes, next free VGPR)}) of csrc/<unit>.hip."""
    out = subprocess.run(["/opt/rocm/bin/hipcc", *makefile_flags(unit), "-S", "--cuda-device-only", "-o", "-", os.path.join(CSRC, unit + ".hip")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.stdout, re.S):
        body = m.group(2)
        kernels[m.group(1)] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                               int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)))
    return out.stdout, kernels
