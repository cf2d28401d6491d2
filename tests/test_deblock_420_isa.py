"""Register / scratch budget of the 4:2:0 deblocking kernels (csrc/deblock_420.hip), read from the gfx950 assembly hipcc emits with the Makefile's
flags (no GPU needed), as tests/test_deblock_isa.py does for csrc/deblock.hip: the unit holds exactly the new kernels, none uses scratch, and none
needs more than 128 VGPRs (four waves per SIMD).  DESIGN.md section 25 records the counts and why the blend is above the 64 of the packed kernels."""
from tests.isa import assemble


def test_deblock_420_unit_holds_the_new_kernels_without_scratch():
    code, kernels = assemble("deblock_420")
    names = " ".join(kernels)
    want = ["k_deblock_down_420ILb0EE", "k_deblock_down_420ILb1EE", "k_deblock_blend_420ILb0EE", "k_deblock_blend_420ILb1EE"]     # I420, NV12
    for k in want:
        assert k in names, k
    assert len(kernels) == len(want)
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 128, f"{name}: {vgprs} VGPRs"
        print(name, vgprs)
    # the blend divides with IEEE rounding (the specification's `num / den`), as k_deblock_blend does
    assert "v_div_fixup_f32" in code


def test_deblock_unit_keeps_exactly_its_own_kernels():
    # tests/test_deblock_isa.py pins the list: 3 pixel sizes x (statistics, downscale, 3 medians) + 3 blends + draw_influence's
    _, kernels = assemble("deblock")
    assert len(kernels) == 3 * (1 + 1 + 3) + 3 + 1 and not [k for k in kernels if "420" in k]
