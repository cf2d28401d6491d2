"""Register / scratch budget of the kernels of lvk_hip_cas_yuv420 / lvk_hip_cas_obs (csrc/cas_420.hip, csrc/cas_obs.hip), read from the gfx950 assembly
hipcc emits with the Makefile's flags (no GPU needed): cas_420 holds exactly its two instances (I420, NV12) and cas_obs exactly its six (one per plane
layout), none uses scratch, none needs more than 128 VGPRs (four waves per SIMD), and the units whose headers they share still hold exactly their own
kernels.  DESIGN.md section 32 records the counts.  A register / scratch budget and nothing else."""
from tests.isa import assemble

SINKS = ["7Sink422ILi0EE", "7Sink422ILi1EE", "7Sink422ILi2EE", "7Sink422ILi3EE", "7Sink444ILi0EE", "7Sink444ILi1EE"]
SRCS = ["6CasSrcILi422ELi0EE", "6CasSrcILi422ELi1EE", "6CasSrcILi422ELi2EE", "6CasSrcILi422ELi3EE", "6CasSrcILi444ELi0EE", "6CasSrcILi444ELi1EE"]


def budget(kernels):
    for name, (scratch, vgprs) in kernels.items():
        print(name, vgprs)
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 128, f"{name}: {vgprs} VGPRs"


def test_cas_420_unit_holds_its_two_instances_without_scratch():
    _, kernels = assemble("cas_420")
    for k in ("k_cas_420ILb0EE", "k_cas_420ILb1EE"):
        assert len([n for n in kernels if k in n]) == 1, k
    assert len(kernels) == 2, sorted(kernels)
    budget(kernels)


def test_cas_obs_unit_holds_its_six_instances_without_scratch():
    _, kernels = assemble("cas_obs")
    want = ["k_cas_obsINS_%sENS_%sE" % (p, s) for p, s in zip(SRCS, SINKS)]
    for k in want:
        assert len([n for n in kernels if k in n]) == 1, k
    assert len(kernels) == len(want) == 6, sorted(kernels)
    budget(kernels)


def test_the_units_that_share_their_headers_keep_exactly_their_own_kernels():
    _, cas = assemble("cas")
    assert len(cas) == 2 and all("k_cas" in k for k in cas), sorted(cas)
    _, cas_gray = assemble("cas_gray")
    assert len(cas_gray) == 1 and all("k_cas_gray" in k for k in cas_gray), sorted(cas_gray)
    _, s420 = assemble("scaling_420")
    assert len(s420) == 4 and all("k_rcas_420" in k for k in s420), sorted(s420)
    _, scaling_obs = assemble("scaling_obs")
    assert len(scaling_obs) == 12 and all("k_rcas_obs" in k for k in scaling_obs), sorted(scaling_obs)
    _, deblock_obs = assemble("deblock_obs")
    assert len(deblock_obs) == 13, sorted(deblock_obs)
    assert not [k for k in list(cas) + list(cas_gray) + list(s420) + list(scaling_obs) + list(deblock_obs) if "k_cas_420" in k or "k_cas_obs" in k]
