"""Register / scratch budget of the fused map remap + 4:2:0 egress kernels (csrc/lens_filter.hip), read from the gfx950 assembly hipcc emits with the
Makefile's flags (no GPU needed): the unit holds exactly the four instances k_remap_map_420[_r1]<false | true>, none uses scratch, none needs more than
128 VGPRs (four waves per SIMD), and DESIGN.md section 27 records the counts the compiler gives."""
import os
import re

from tests.isa import ROOT, assemble

WANT = {"k_remap_map_420ILb0EE": "k_remap_map_420<false>", "k_remap_map_420ILb1EE": "k_remap_map_420<true>",
        "k_remap_map_420_r1ILb0EE": "k_remap_map_420_r1<false>", "k_remap_map_420_r1ILb1EE": "k_remap_map_420_r1<true>"}


def test_lens_filter_unit_holds_the_four_instances_without_scratch():
    _, kernels = assemble("lens_filter")
    assert len(kernels) == len(WANT), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 27."):]
    for mangled, plain in WANT.items():
        found = [k for k in kernels if mangled in k]
        assert len(found) == 1, mangled
        scratch, vgprs = kernels[found[0]]
        print(plain, vgprs)
        assert scratch == 0, f"{plain}: {scratch} bytes of scratch"
        assert vgprs <= 128, f"{plain}: {vgprs} VGPRs"
        row = re.search(r"^\| `%s` \| (\d+) \|" % re.escape(plain), section, re.M)
        assert row and int(row.group(1)) == vgprs, f"{plain}: {vgprs} VGPRs, DESIGN.md section 27 says {row and row.group(1)}"


def test_remap_unit_keeps_its_own_kernels():
    _, kernels = assemble("remap")
    assert not [k for k in kernels if "k_remap_map_420" in k]
    assert [k for k in kernels if "k_remap_mapILb1EE" in k] and [k for k in kernels if "k_remap_mesh_420ILb0EE" in k]
