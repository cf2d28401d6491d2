"""Register / scratch budget of the deblocking kernels (csrc/deblock.hip), read from the gfx950 assembly hipcc emits with the Makefile's
flags (no GPU needed), as tests/test_isa_budget.py does for the other units: no kernel may use scratch, and the bandwidth-bound kernels
stay small enough for full occupancy (<= 64 VGPRs: 8 waves per SIMD)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livevisionkit_amd", "csrc")


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS = (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    return [f.replace("-I../../include", "-I" + os.path.join(ROOT, "include")).replace("-I.", "-I" + CSRC) if f.startswith("-I") else f
            for f in flags]


def test_deblock_kernels_use_no_scratch():
    out = subprocess.run(["/opt/rocm/bin/hipcc", *_makefile_flags(), "-S", "--cuda-device-only", "-o", "-", os.path.join(CSRC, "deblock.hip")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.stdout, re.S):
        body = m.group(2)
        kernels[m.group(1)] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                               int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)))
    names = " ".join(kernels)
    for k in ("k_deblock_stats", "k_deblock_down", "k_deblock_median", "k_deblock_blend"):
        assert k in names, k
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 64, f"{name}: {vgprs} VGPRs"
    # the blend divides with IEEE rounding (the specification's `num / den`), not with the approximate reciprocal
    assert "v_div_fixup_f32" in out.stdout
