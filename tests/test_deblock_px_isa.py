"""Register / scratch budget of the one- and four-channel deblocking kernels (csrc/deblock_px.hip), read from the gfx950 assembly hipcc emits with the
Makefile's flags (no GPU needed), as tests/test_deblock_isa.py does for the three-channel unit: no scratch, <= 64 VGPRs (8 waves per SIMD)."""
from tests.isa import assemble


def test_deblock_px_kernels_use_no_scratch():
    code, kernels = assemble("deblock_px")
    names = " ".join(kernels)
    for k in ("k_deblock_stats_px", "k_deblock_down_px", "k_deblock_median_px", "k_deblock_blend_c4", "k_deblock_blend_gray"):
        assert k in names, k
    assert len(kernels) == 2 + 2 + 6 + 2          # stats, down and median (k = 3, 5, run-time) for both pixel sizes, one blend each
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 64, f"{name}: {vgprs} VGPRs"
    # the blend divides with IEEE rounding (the specification's `num / den`), not with the approximate reciprocal
    assert "v_div_fixup_f32" in code
