"""Register / scratch budget and instruction choices of the FSR EASU kernels (csrc/fsr.hip), read from the gfx950 assembly hipcc emits with
the Makefile's flags (no GPU needed), as tests/test_cas_isa.py does for CAS: no scratch, at most 128 VGPRs, the FidelityFX integer tricks for
the approximate reciprocals and inverse square root (no v_sqrt_f32 / v_rsq_f32), and min3 / max3 for the deringing clamp."""
from tests.isa import assemble


def test_fsr_kernels_budget_and_instructions():
    code, kernels = assemble("fsr")
    assert len(kernels) == 4 and all("k_fsr_easu" in k for k in kernels), sorted(kernels)   # <3 | 4, staged | direct>
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 128, f"{name}: {vgprs} VGPRs"
    for banned in ("v_sqrt_f32", "v_rsq_f32", "scratch_"):
        assert banned not in code, banned
    # per kernel: three channels of min(min3(f, g, j), k) and max(max3(f, g, j), k)
    assert code.count("v_min3_f32") >= 12 and code.count("v_max3_f32") >= 12
