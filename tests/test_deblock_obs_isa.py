"""Register / scratch budget of the kernels of lvk_hip_deblock_apply_obs (csrc/deblock_obs.hip), read from the gfx950 assembly hipcc emits with the
Makefile's flags (no GPU needed): the unit holds exactly its thirteen instances -- the strided-luma statistics, and the downscale and the blend for
each of the six plane layouts --, none uses scratch, none needs more than 128 VGPRs (four waves per SIMD), and the units it shares headers with still
hold exactly their own kernels.  DESIGN.md section 31 records the counts.  A register / scratch budget and nothing else."""
from tests.isa import assemble

SINKS = ["7Sink422ILi0EE", "7Sink422ILi1EE", "7Sink422ILi2EE", "7Sink422ILi3EE", "7Sink444ILi0EE", "7Sink444ILi1EE"]
SRCS = ["6ObsSrcILi422ELi0EE", "6ObsSrcILi422ELi1EE", "6ObsSrcILi422ELi2EE", "6ObsSrcILi422ELi3EE", "6ObsSrcILi444ELi0EE", "6ObsSrcILi444ELi1EE"]


def test_deblock_obs_unit_holds_its_thirteen_instances_without_scratch():
    _, kernels = assemble("deblock_obs")
    want = (["k_deblock_stats_luma"] + ["k_deblock_down_obsINS_%sE" % s for s in SRCS]
            + ["k_deblock_blend_obsINS_%sENS_%sE" % (p, s) for p, s in zip(SRCS, SINKS)])
    for k in want:
        assert len([n for n in kernels if k in n]) == 1, k
    assert len(kernels) == len(want) == 13, sorted(kernels)
    for name, (scratch, vgprs) in kernels.items():
        print(name, vgprs)
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 128, f"{name}: {vgprs} VGPRs"


def test_the_units_that_share_its_headers_keep_exactly_their_own_kernels():
    _, deblock = assemble("deblock")
    assert len(deblock) == 19 and all("k_deblock_" in k for k in deblock), sorted(deblock)
    _, d420 = assemble("deblock_420")
    assert len(d420) == 4 and all("k_deblock_down_420" in k or "k_deblock_blend_420" in k for k in d420), sorted(d420)
    _, scaling_obs = assemble("scaling_obs")
    assert len(scaling_obs) == 12 and all("k_rcas_obs" in k for k in scaling_obs), sorted(scaling_obs)
    _, remap_obs = assemble("remap_obs")
    assert len(remap_obs) == 60, len(remap_obs)
    assert not [k for k in list(deblock) + list(d420) + list(scaling_obs) + list(remap_obs) if "_obsINS_6ObsSrc" in k or "k_deblock_stats_luma" in k]
