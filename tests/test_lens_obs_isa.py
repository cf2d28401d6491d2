"""Register / scratch budget of the materialised-map remap with an OBS sink (k_remap_map_planes, csrc/remap_obs.hip), read from the gfx950 assembly
hipcc emits with the Makefile's flags (no GPU needed): the unit holds k_remap_map_planes and its `_r1` twin for exactly the six sinks beside its four
existing families, no kernel of the unit uses scratch, the new instances need at most 128 VGPRs (four waves per SIMD), DESIGN.md section 29 records
the VGPR and instruction counts the compiler gives, and lens_filter.hip, which holds the entries, still holds its four kernels."""
import os
import re

from tests.isa import ROOT, assemble

SINKS = {"7Sink422ILi0EE": "Sink422<0>", "7Sink422ILi1EE": "Sink422<1>", "7Sink422ILi2EE": "Sink422<2>", "7Sink422ILi3EE": "Sink422<3>",
         "7Sink444ILi0EE": "Sink444<0>", "7Sink444ILi1EE": "Sink444<1>"}
FAMILIES = ["k_remap_homography_planes", "k_remap_homography_lens_planes", "k_remap_mesh_planes", "k_remap_mesh_lens_planes", "k_remap_map_planes"]


def family_of(mangled):
    return re.search(r"\d+(k_\w+?)INS", mangled).group(1)


def instances():
    """{(family, sink): (mangled name, scratch, vgprs, static instructions)} of remap_obs.hip"""
    code, kernels = assemble("remap_obs")
    out = {}
    for mangled, (scratch, vgprs) in kernels.items():
        sink = [plain for tag, plain in SINKS.items() if tag in mangled]
        assert len(sink) == 1, mangled
        body = re.search(r"^%s:[^\n]*\n(.*?)\.Lfunc_end" % re.escape(mangled), code, re.S | re.M).group(1)
        ops = [ln.split()[0] for ln in body.splitlines() if ln.strip() and not ln.strip().startswith((";", ".", "//")) and not ln.strip().endswith(":")]
        out[(family_of(mangled), sink[0])] = (mangled, scratch, vgprs, len(ops))
    return out


def test_remap_obs_holds_the_map_family_for_the_six_sinks_beside_its_four_families():
    found = instances()
    want = {(f + tail, s) for f in FAMILIES for tail in ("", "_r1") for s in SINKS.values()}
    assert set(found) == want, sorted(set(found) ^ want)
    for (family, sink), (_, scratch, vgprs, _) in found.items():
        assert scratch == 0, f"{family}<{sink}>: {scratch} bytes of scratch"


def test_new_instances_fit_four_waves_and_design_records_their_counts():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 29."):]
    for (family, sink), (_, scratch, vgprs, ops) in sorted(instances().items()):
        if not family.startswith("k_remap_map_planes"):
            continue
        plain = "%s<%s>" % (family, sink)
        print(plain, vgprs, ops)
        assert vgprs <= 128, f"{plain}: {vgprs} VGPRs"
        row = re.search(r"^\| `%s` \| (\d+) \| (\d+) \|" % re.escape(plain), section, re.M)
        assert row, f"{plain}: no row in DESIGN.md section 29"
        assert (int(row.group(1)), int(row.group(2))) == (vgprs, ops), f"{plain}: {vgprs} VGPRs, {ops} instructions; DESIGN.md section 29 says {row.group(1)}, {row.group(2)}"


def test_lens_filter_still_holds_its_four_kernels():
    _, kernels = assemble("lens_filter")
    assert len(kernels) == 4 and all("k_remap_map_420" in k for k in kernels), sorted(kernels)
