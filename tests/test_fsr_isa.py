"""Register / scratch budget and instruction choices of the FSR EASU kernels (csrc/fsr.hip), read from the gfx950 assembly hipcc emits with
the Makefile's flags (no GPU needed), as tests/test_cas_isa.py does for CAS: no scratch, at most 128 VGPRs, the FidelityFX integer tricks for
the approximate reciprocals and inverse square root (no v_sqrt_f32 / v_rsq_f32), and min3 / max3 for the deringing clamp."""
import os
import re
import subprocess

from tests.test_cas_isa import CSRC, _makefile_flags


def test_fsr_kernels_budget_and_instructions():
    out = subprocess.run(["/opt/rocm/bin/hipcc", *_makefile_flags(), "-S", "--cuda-device-only", "-o", "-", os.path.join(CSRC, "fsr.hip")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.stdout, re.S):
        body = m.group(2)
        kernels[m.group(1)] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                               int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)))
    assert len(kernels) == 4 and all("k_fsr_easu" in k for k in kernels), sorted(kernels)   # <3 | 4, staged | direct>
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 128, f"{name}: {vgprs} VGPRs"
    code = out.stdout
    for banned in ("v_sqrt_f32", "v_rsq_f32", "scratch_"):
        assert banned not in code, banned
    # per kernel: three channels of min(min3(f, g, j), k) and max(max3(f, g, j), k)
    assert code.count("v_min3_f32") >= 12 and code.count("v_max3_f32") >= 12
