"""Register / scratch budget of the deblocking kernels (csrc/deblock.hip: one-, three- and four-channel frames), read from the gfx950 assembly
hipcc emits with the Makefile's flags (no GPU needed), as tests/test_isa_budget.py does for the other units: no kernel may use scratch, and
the bandwidth-bound kernels stay small enough for full occupancy (<= 64 VGPRs: 8 waves per SIMD)."""
from tests.isa import assemble


def test_deblock_kernels_of_every_pixel_size_use_no_scratch():
    code, kernels = assemble("deblock")
    names = " ".join(kernels)
    # every kernel family for each pixel size it is built for (template arguments as the mangled names spell them)
    want = ["k_deblock_blend_gray", "k_deblock_blendILi3ELb0EE", "k_deblock_blendILi4ELb0EE", "k_deblock_blendILi3ELb1EE"]       # the last: draw_influence
    for bpp in (1, 3, 4):
        want += ["k_deblock_statsILi%dEE" % bpp, "k_deblock_downILi%dEE" % bpp] + ["k_deblock_medianILi%dELi%dEE" % (bpp, ks) for ks in (3, 5, 0)]
    for k in want:
        assert k in names, k
    assert len(kernels) == len(want) == 3 * (1 + 1 + 3) + 3 + 1
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 64, f"{name}: {vgprs} VGPRs"
    # the blend divides with IEEE rounding (the specification's `num / den`), not with the approximate reciprocal
    assert "v_div_fixup_f32" in code
