"""Register / scratch budget and instruction choices of the CAS kernels (csrc/cas.hip), read from the gfx950 assembly hipcc emits with the
Makefile's flags (no GPU needed), as tests/test_deblock_isa.py does for the deblocking kernels: no scratch, at most 96 VGPRs, min3 / max3
for the neighbourhood and the FidelityFX integer tricks for the reciprocals and the square root (no v_sqrt_f32 / v_rsq_f32)."""
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


def test_cas_kernels_budget_and_instructions():
    out = subprocess.run(["/opt/rocm/bin/hipcc", *_makefile_flags(), "-S", "--cuda-device-only", "-o", "-", os.path.join(CSRC, "cas.hip")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.stdout, re.S):
        body = m.group(2)
        kernels[m.group(1)] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                               int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)))
    assert len(kernels) == 2 and all("k_cas" in k for k in kernels), sorted(kernels)       # k_cas<3>, k_cas<4>
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 96, f"{name}: {vgprs} VGPRs"
    code = out.stdout
    for banned in ("v_sqrt_f32", "v_rsq_f32", "v_rcp_f32", "v_div_fixup_f32", "scratch_"):
        assert banned not in code, banned
    assert "v_min3_f32" in code and "v_max3_f32" in code
