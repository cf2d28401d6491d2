"""Register / scratch budget of the one-channel CAS and FSR EASU kernels (csrc/cas_gray.hip, csrc/fsr_gray.hip), read from the gfx950 assembly
hipcc emits with the Makefile's flags (no GPU needed): no scratch and no more VGPRs than the budgets of their three-channel siblings, 96 for CAS
and 128 for EASU.  The per-pixel arithmetic of both families lives in csrc/cas_core.hpp and csrc/fsr_core.hpp, so the three-channel units are
assembled again here: their kernels are still 2 and 4, within the same budgets."""
import os

import pytest

from tests.isa import CSRC, assemble

BUDGET = {"cas": 96, "cas_gray": 96, "fsr": 128, "fsr_gray": 128}
KERNELS = {"cas": (2, "k_cas"), "cas_gray": (1, "k_cas_gray"), "fsr": (4, "k_fsr_easu"), "fsr_gray": (2, "k_fsr_easu_gray")}


@pytest.mark.parametrize("unit", sorted(BUDGET))
def test_kernels_names_count_scratch_and_vgprs(unit):
    code, kernels = assemble(unit)
    count, stem = KERNELS[unit]
    assert len(kernels) == count and all(stem in k for k in kernels), sorted(kernels)
    if not unit.endswith("_gray"):
        assert not any("gray" in k for k in kernels), sorted(kernels)
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= BUDGET[unit], f"{name}: {vgprs} VGPRs"
    for banned in ("v_sqrt_f32", "v_rsq_f32", "scratch_"):
        assert banned not in code, banned


def test_gray_kernels_use_the_shared_arithmetic():
    """The gray units hold no copy of the arithmetic: they include the headers the three-channel units include, and the FidelityFX constants
    appear in the headers only."""
    for unit, core in (("cas", "cas_core.hpp"), ("cas_gray", "cas_core.hpp"), ("fsr", "fsr_core.hpp"), ("fsr_gray", "fsr_core.hpp")):
        text = open(os.path.join(CSRC, unit + ".hip")).read()
        assert '#include "%s"' % core in text, unit
        for constant in ("0x7ef07ebb", "0x7ef19fff", "0x5f347d74", "0x1fbc4639"):
            assert constant not in text, (unit, constant)
    code, _ = assemble("cas_gray")
    assert "v_min3_f32" in code and "v_max3_f32" in code and "v_rcp_f32" not in code
    code, _ = assemble("fsr_gray")
    assert "v_min3_f32" in code and "v_max3_f32" in code
