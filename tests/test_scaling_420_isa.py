"""Register / scratch budget of the 4:2:0 sharpening kernel (csrc/scaling_420.hip), read from the gfx950 assembly hipcc emits with the Makefile's flags
(no GPU needed): the unit holds exactly the four instances of k_rcas_420 -- two sources, two layouts --, none uses scratch, and none needs more than
128 VGPRs (four waves per SIMD).  DESIGN.md section 26 records the counts."""
from tests.isa import assemble


def test_scaling_420_unit_holds_the_four_instances_without_scratch():
    _, kernels = assemble("scaling_420")
    names = " ".join(kernels)
    want = ["k_rcas_420INS_9PlanarSrcILb0EEELb0EE", "k_rcas_420INS_9PlanarSrcILb1EEELb1EE", "k_rcas_420INS_9PackedSrcELb0EE", "k_rcas_420INS_9PackedSrcELb1EE"]
    for k in want:
        assert k in names, k
    assert len(kernels) == len(want)
    for name, (scratch, vgprs) in kernels.items():
        print(name, vgprs)
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 128, f"{name}: {vgprs} VGPRs"


def test_sharpen_unit_keeps_exactly_its_own_kernels():
    _, kernels = assemble("sharpen")
    assert len(kernels) == 2 and [k for k in kernels if "k_rcasILi4EE" in k] and [k for k in kernels if "k_native_rcp" in k]
    assert not [k for k in kernels if "420" in k]
    for name, (scratch, _) in kernels.items():
        assert scratch == 0, name
