"""Register / scratch / LDS budget of the kernels of lvk_hip_fsr_yuv420 / lvk_hip_fsr_obs (csrc/fsr_420.hip, csrc/fsr_obs.hip: the instances of k_fsr_planes
of csrc/fsr_planes.hpp), read from the gfx950 assembly hipcc emits with the Makefile's flags (no GPU needed): fsr_420 holds exactly its four instances
(I420 / NV12 out, staged from the planes / direct from a packed frame) and fsr_obs exactly its twelve (one staged and one direct per plane layout), none
uses scratch, none needs more than 128 VGPRs (four waves per SIMD), none declares more than 40 KiB of LDS (four blocks per CU), and fsr and fsr_gray,
whose pixel function moved into fsr_core.hpp, still hold exactly their own kernels.  DESIGN.md section 33 records the counts.  A register / scratch /
LDS budget and nothing else."""
import re

from tests.isa import assemble

SINKS = ["7Sink422ILi0EE", "7Sink422ILi1EE", "7Sink422ILi2EE", "7Sink422ILi3EE", "7Sink444ILi0EE", "7Sink444ILi1EE"]
SRCS = ["6FsrSrcILi422ELi0EE", "6FsrSrcILi422ELi1EE", "6FsrSrcILi422ELi2EE", "6FsrSrcILi422ELi3EE", "6FsrSrcILi444ELi0EE", "6FsrSrcILi444ELi1EE"]
LDS_BUDGET = 40 * 1024


def lds_of(code):
    """kernel name -> bytes of static LDS (.amdhsa_group_segment_fixed_size of its kernel descriptor)"""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", code)}


def budget(code, kernels):
    lds = lds_of(code)
    assert sorted(lds) == sorted(kernels), (sorted(lds), sorted(kernels))
    for name, (scratch, vgprs) in kernels.items():
        print(name, vgprs, lds[name])
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 128, f"{name}: {vgprs} VGPRs"
        assert lds[name] <= LDS_BUDGET, f"{name}: {lds[name]} bytes of LDS"
        staged = re.search(r"Lb([01])EEEv", name).group(1) == "1"                   # the last template argument
        assert lds[name] == (LDS_BUDGET if staged else 4096), f"{name}: {lds[name]} bytes of LDS (the stage with the out-tile inside it | the out-tile)"


def test_fsr_420_unit_holds_its_four_instances_within_the_budget():
    code, kernels = assemble("fsr_420")
    want = ["k_fsr_planesINS_6Src420ILb0EEENS_6Out420ILb0EEELb1EE", "k_fsr_planesINS_6Src420ILb1EEENS_6Out420ILb1EEELb1EE",
            "k_fsr_planesINS_9PackedYuvENS_6Out420ILb0EEELb0EE", "k_fsr_planesINS_9PackedYuvENS_6Out420ILb1EEELb0EE"]
    for k in want:
        assert len([n for n in kernels if k in n]) == 1, (k, sorted(kernels))
    assert len(kernels) == len(want) == 4, sorted(kernels)
    budget(code, kernels)


def test_fsr_obs_unit_holds_its_twelve_instances_within_the_budget():
    code, kernels = assemble("fsr_obs")
    want = ["k_fsr_planesINS_%sENS_7SinkOutINS_%sEEELb1EE" % (p, s) for p, s in zip(SRCS, SINKS)]
    want += ["k_fsr_planesINS_9PackedYuvENS_7SinkOutINS_%sEEELb0EE" % s for s in SINKS]
    for k in want:
        assert len([n for n in kernels if k in n]) == 1, (k, sorted(kernels))
    assert len(kernels) == len(want) == 12, sorted(kernels)
    budget(code, kernels)


def test_the_units_that_share_their_headers_keep_exactly_their_own_kernels():
    _, fsr = assemble("fsr")
    assert len(fsr) == 4 and all("k_fsr_easu" in k for k in fsr), sorted(fsr)
    _, fsr_gray = assemble("fsr_gray")
    assert len(fsr_gray) == 2 and all("k_fsr_easu_gray" in k for k in fsr_gray), sorted(fsr_gray)
    assert not [k for k in list(fsr) + list(fsr_gray) if "k_fsr_planes" in k]
