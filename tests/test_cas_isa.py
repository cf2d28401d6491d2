"""Register / scratch budget and instruction choices of the CAS kernels (csrc/cas.hip), read from the gfx950 assembly hipcc emits with the
Makefile's flags (no GPU needed), as tests/test_deblock_isa.py does for the deblocking kernels: no scratch, at most 96 VGPRs, min3 / max3
for the neighbourhood and the FidelityFX integer tricks for the reciprocals and the square root (no v_sqrt_f32 / v_rsq_f32)."""
from tests.isa import assemble


def test_cas_kernels_budget_and_instructions():
    code, kernels = assemble("cas")
    assert len(kernels) == 2 and all("k_cas" in k for k in kernels), sorted(kernels)       # k_cas<3>, k_cas<4>
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 96, f"{name}: {vgprs} VGPRs"
    for banned in ("v_sqrt_f32", "v_rsq_f32", "v_rcp_f32", "v_div_fixup_f32", "scratch_"):
        assert banned not in code, banned
    assert "v_min3_f32" in code and "v_max3_f32" in code
