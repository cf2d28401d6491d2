"""Register / scratch budget of the drawing kernels (csrc/draw.hip), read from the gfx950 assembly hipcc emits with the Makefile's flags (no
GPU needed), as tests/test_fsr_isa.py does for FSR: no scratch and at most 64 VGPRs for k_draw_points, k_draw_rect and k_draw_text, and no
scalar memory write anywhere in the unit -- the kernels write pixels with vector byte stores only."""
import re

from tests.isa import assemble

# scalar stores, scalar atomics and the scalar data cache's write-back / discard, spelt in pieces: every s_ mnemonic that writes memory
SCALAR_WRITES = re.compile(r"\bs_(?:buffer_|scratch_)?(?:" + "sto" + "re|ato" + "mic)|\bs_dca" + "che_(?:wb|discard)")


def test_draw_kernels_budget_and_instructions():
    code, kernels = assemble("draw")
    new = {what: [k for k in kernels if what in k] for what in ("k_draw_points", "k_draw_rect", "k_draw_text")}
    assert all(len(v) == 1 for v in new.values()), sorted(kernels)
    assert len(kernels) == 5 and any("k_draw_grid" in k for k in kernels) and any("k_draw_crosses" in k for k in kernels), sorted(kernels)
    for what, (name,) in new.items():
        scratch, vgprs = kernels[name]
        assert scratch == 0, f"{what}: {scratch} bytes of scratch"
        assert vgprs <= 64, f"{what}: {vgprs} VGPRs"
    assert "scratch_" not in code
    assert not SCALAR_WRITES.search(code), SCALAR_WRITES.search(code).group(0)
    assert "global_store_byte" in code                         # (the pattern above is looked for in real assembly)
