"""The one- and four-channel upscale and RCAS kernels in the gfx950 assembly (no GPU needed): none of them uses scratch, and k_easu_scale_px stays within the
80 VGPRs of every kernel that runs the remap strip body (tests/test_isa_budget.py).  The RCAS kernels' VGPR counts are printed and recorded in DESIGN.md
section 22, not asserted."""
import re

from tests.isa import assemble


def _kernels(unit, base):
    found = {k: v for k, v in assemble(unit)[1].items() if re.search(r"\d+" + base + "I", k)}
    assert len(found) == 2, (unit, base, list(assemble(unit)[1]))           # the GRAY and the four-channel instantiation
    return found


def test_the_upscale_kernels_use_no_scratch_and_at_most_80_vgprs():
    for name, (scratch, vgprs) in _kernels("remap_px", "k_easu_scale_px").items():
        print(f"{name}: {vgprs} VGPRs")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 80, f"{name}: {vgprs} VGPRs (budget 80)"


def test_the_rcas_kernels_use_no_scratch():
    for name, (scratch, vgprs) in _kernels("sharpen_px", "k_rcas_px").items():
        print(f"{name}: {vgprs} VGPRs")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
