"""Register / scratch budget and memory instructions of the format conversion kernels (csrc/convert.hip), read from the gfx950 assembly hipcc
emits with the Makefile's flags (no GPU needed), as tests/test_cas_isa.py does for CAS: no scratch, at most 64 VGPRs, and the interior-path
kernels move their bytes as whole dwords (dwordx4 / dwordx3), never a byte at a time, with v_perm_b32 for the byte moves."""
import re

from tests.isa import assemble

MAP_OPS = {0, 1, 2, 3, 4}          # OP_KEEP, OP_SWAP, OP_REP, OP_Y, OP_G2YUV: byte moves only


def test_convert_kernels_budget_and_instructions():
    code, kernels = assemble("convert")
    # 22 (source channels, destination channels, operation) instantiations, each with an interior and a general kernel
    assert len(kernels) == 44 and all("k_convert_" in k for k in kernels), sorted(kernels)
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgprs <= 64, f"{name}: {vgprs} VGPRs"
    assert "scratch_" not in code
    bodies = dict(re.findall(r"^(_ZN\S+k_convert_\S+):.*?$(.*?)^\.Lfunc_end", code, re.M | re.S))
    interior = {k: v for k, v in bodies.items() if "k_convert_interior" in k}
    assert len(interior) == 22
    for name, body in interior.items():
        sc, dc, op = map(int, re.search(r"k_convert_interiorILi(\d)ELi(\d)ELi(\d+)E", name).groups())
        loads = re.findall(r"global_load_dword(x[34])?\b", body)
        stores = re.findall(r"global_store_dword(x[34])?\b", body)
        assert loads and all(x for x in loads), f"{name}: loads {loads}"
        assert stores and all(x for x in stores), f"{name}: stores {stores}"
        for banned in ("global_load_ubyte", "global_load_ushort", "global_store_byte", "global_store_short", "flat_"):
            assert banned not in body, f"{name}: {banned}"
        if op in MAP_OPS:
            assert "v_perm_b32" in body, name
        else:
            assert re.search(r"v_ma[dc]\w*_[iu]32_[iu]24|v_mul_[iu]32_[iu]24", body), f"{name}: no 24-bit multiply-add"
    general = [k for k in bodies if "k_convert_general" in k]
    assert len(general) == 22
