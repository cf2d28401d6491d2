"""Register / scratch budget of the deblocking kernels (csrc/deblock.hip), read from the gfx950 assembly hipcc emits with the Makefile's
flags (no GPU needed), as tests/test_isa_budget.py does for the other units: no kernel may use scratch, and the bandwidth-bound kernels
stay small enough for full occupancy (<= 64 VGPRs: 8 waves per SIMD)."""
from tests.isa import assemble


def test_deblock_kernels_use_no_scratch():
    code, kernels = assemble("deblock")
    names = " ".join(kernels)
    for k in ("k_deblock_stats", "k_deblock_down", "k_deblock_median", "k_deblock_blend"):
        assert k in names, k
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 64, f"{name}: {vgprs} VGPRs"
    # the blend divides with IEEE rounding (the specification's `num / den`), not with the approximate reciprocal
    assert "v_div_fixup_f32" in code
