"""Register / scratch budget of the sharpening kernel that writes an OBS format's planes (k_rcas_obs, csrc/scaling_obs.hip), read from the gfx950 assembly
hipcc emits with the Makefile's flags (no GPU needed): the unit holds exactly the twelve instances -- the packed source and the plane source for each of
the six sinks --, none uses scratch, none needs more than 128 VGPRs (four waves per SIMD), and the units it shares headers with still hold exactly their
own kernels.  DESIGN.md section 30 records the counts.  A register / scratch budget and nothing else."""
from tests.isa import assemble

SINKS = ["7Sink422ILi0EE", "7Sink422ILi1EE", "7Sink422ILi2EE", "7Sink422ILi3EE", "7Sink444ILi0EE", "7Sink444ILi1EE"]
PLANE_SRC = ["8PlaneSrcILi422ELi0EE", "8PlaneSrcILi422ELi1EE", "8PlaneSrcILi422ELi2EE", "8PlaneSrcILi422ELi3EE", "8PlaneSrcILi444ELi0EE", "8PlaneSrcILi444ELi1EE"]


def test_scaling_obs_unit_holds_the_twelve_instances_without_scratch():
    _, kernels = assemble("scaling_obs")
    want = ["k_rcas_obsINS_9PackedSrcENS_%sE" % s for s in SINKS] + ["k_rcas_obsINS_%sENS_%sE" % (p, s) for p, s in zip(PLANE_SRC, SINKS)]
    for k in want:
        assert len([n for n in kernels if k in n]) == 1, k
    assert len(kernels) == len(want) == 12, sorted(kernels)
    for name, (scratch, vgprs) in kernels.items():
        print(name, vgprs)
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 128, f"{name}: {vgprs} VGPRs"


def test_the_units_that_share_its_headers_keep_exactly_their_own_kernels():
    _, k420 = assemble("scaling_420")
    assert len(k420) == 4 and all("k_rcas_420" in k for k in k420), sorted(k420)
    _, sharpen = assemble("sharpen")
    assert len(sharpen) == 2 and [k for k in sharpen if "k_rcasILi4EE" in k] and [k for k in sharpen if "k_native_rcp" in k]
    _, remap_obs = assemble("remap_obs")
    assert len(remap_obs) == 60 and all("k_remap_" in k and "planes" in k for k in remap_obs), len(remap_obs)
    assert not [k for k in list(k420) + list(sharpen) + list(remap_obs) if "k_rcas_obs" in k]
