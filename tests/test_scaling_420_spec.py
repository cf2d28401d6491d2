"""CPU side of lvk_hip_scale_yuv420: the symbol's surface, the closed form of the chroma up-sampling the planar kernel uses, and the
conditions under which a pass of the GPU tests (tests/test_scaling_420_gpu.py) means something -- the cases of tests/scaling_420_cases.py are live: the
sharpening changes the planes, the up-scaling is no nearest-neighbour copy and runs the YUV program, the ends of the sharpness range differ, and the
chroma at equal sizes is no copy of the input.  The thresholds sit below the smallest values seen with the two textures at seed 7; they are
conditions on the cases, not tolerances on the code."""
import os
import re

import numpy as np
import pytest

from tests.scaling_420_cases import (C_2x2, C_4x4, CASES, SHARPNESS_ENDS, TEXTURES, as_nv12, case_id, chain, equal_sizes, expected, oracle)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARGS = ["const void* d_y", "int y_step", "const void* d_u", "int u_step", "const void* d_v", "int v_step", "int src_rows", "int src_cols",
        "void* o_y", "int oy_step", "void* o_u", "int ou_step", "void* o_v", "int ov_step", "int dst_rows", "int dst_cols", "int nv12", "float sharpness"]


def test_symbol_is_declared_bound_and_exported():
    """include/lvk_hip_scaling_420.h declares exactly the entry, lvk_hip.h includes it in its PART 2 (inside its include guard, behind its own
    declarations, next to the two deblock headers), and livevisionkit_amd/_native.py binds exactly what it declares."""
    import ctypes
    from livevisionkit_amd import _native
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvk_hip_scaling_420.h")).read(), flags=re.S)
    assert re.findall(r"\b(lvk_(?:hip|stab)_[a-z0-9_]+)\s*\(", code) == ["lvk_hip_scale_yuv420"] == _native.symbols_scaling_420()
    decl = re.search(r"^int lvk_hip_scale_yuv420\(lvk_hip_ctx\* ctx,(.*?)\);", code, re.S | re.M)
    assert decl and [a.strip() for a in decl.group(1).replace("\n", " ").split(",")] == ARGS
    text = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    assert re.search(r'^#include "lvk_hip_scaling_420.h"', experimental, re.M) and "lvk_hip_scaling_420.h" not in stable
    # at the header's end, inside its include guard, next to the two deblock headers
    tail = text[text.rindex("#ifdef __cplusplus"):]
    assert [h for h in re.findall(r'^#include "(.*?)"', tail, re.M)] == ["lvk_hip_scaling_420.h", "lvk_hip_deblock_420.h", "lvk_hip_deblock_px.h"]
    assert tail.rstrip().endswith("#endif /* LVK_HIP_H */")
    assert "lvk_hip_scale_yuv420" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fn = _native.load().lvk_hip_scale_yuv420
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 1 + len(ARGS)
    assert fn(None, *([None, 0] * 3), 0, 0, *([None, 0] * 3), 0, 0, 0, 0.5) != 0       # a NULL context is refused before anything is touched
    import livevisionkit_amd as lvk
    assert callable(lvk.Context.scale_yuv420)


def test_the_header_is_plain_c_either_way_round(tmp_path):
    """C99 with -pedantic, whichever of the two headers a host includes first."""
    import subprocess
    for first, second in (("lvk_hip.h", "lvk_hip_scaling_420.h"), ("lvk_hip_scaling_420.h", "lvk_hip.h")):
        src = tmp_path / "s420.c"
        src.write_text('#include "%s"\n#include "%s"\n'
                       'int main(void) { (void)lvk_hip_scale_yuv420; (void)lvk_hip_sharpen; return 0; }\n' % (first, second))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_the_makefile_rule_lists_the_new_headers():
    rule = re.search(r"^%\.o: %\.hip (.*)$", open(os.path.join(ROOT, "livevisionkit_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    for h in ("rcas_core.hpp", "yuv420_core.hpp", "../../include/lvk_hip_scaling_420.h"):
        assert h in rule, h


@pytest.mark.parametrize("kind", TEXTURES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_i420_and_the_same_samples_as_nv12_give_the_same_specification(case, kind):
    o = oracle()
    e = expected(case, kind)
    assert np.array_equal(o.ingest_yuv420(*as_nv12(e["planes"])), e["packed"])
    if equal_sizes(case):
        assert np.array_equal(e["scaled"], e["packed"])                                  # lvk::upscale copies (Image.cpp:162-166)
    y, uv = o.egress_yuv420(o.sharpen(e["scaled"], case[4]), nv12=True)
    assert np.array_equal(y, e["want"][0]) and np.array_equal(uv[..., 0], e["want"][1]) and np.array_equal(uv[..., 1], e["want"][2])


def up_closed_form(c):
    """The 2x up-sampling as csrc/yuv420_core.hpp restates it from the comment above k_ingest_yuv420_x2: t = 3 C[c] + C[f] horizontally,
    (((3 t_k) >> 2) + (t_g >> 2) + 2) >> 2 vertically, f / g the outer neighbour of the sample, clamped to the plane."""
    c = c.astype(np.int64)
    cr, cc = c.shape
    x, y = np.arange(2 * cc), np.arange(2 * cr)
    near_x, far_x = x // 2, np.clip(np.where(x & 1, x // 2 + 1, x // 2 - 1), 0, cc - 1)
    near_y, far_y = y // 2, np.clip(np.where(y & 1, y // 2 + 1, y // 2 - 1), 0, cr - 1)
    t = 3 * c[:, near_x] + c[:, far_x]
    return (((3 * t[near_y]) >> 2) + (t[far_y] >> 2) + 2) >> 2


def up_both_planes_at_once(u, v):
    """The same with U's sums in the low and V's in the high 16 bits of one word, as PlanarSrc (csrc/scaling_420.hip) keeps them: 3 t <= 3060 stays
    inside its half, and the two bits a right shift moves across the halves are masked off."""
    cr, cc = u.shape
    s = u.astype(np.int64) | (v.astype(np.int64) << 16)
    x, y = np.arange(2 * cc), np.arange(2 * cr)
    near_x, far_x = x // 2, np.clip(np.where(x & 1, x // 2 + 1, x // 2 - 1), 0, cc - 1)
    near_y, far_y = y // 2, np.clip(np.where(y & 1, y // 2 + 1, y // 2 - 1), 0, cr - 1)
    t = 3 * s[:, near_x] + s[:, far_x]
    uv = ((((3 * t[near_y]) >> 2) & 0x3fff3fff) + ((t[far_y] >> 2) & 0x3fff3fff) + 0x00020002) >> 2
    return uv & 0xff, (uv >> 16) & 0xff


@pytest.mark.parametrize("kind", TEXTURES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_closed_form_of_the_up_sampling_is_the_ingest(case, kind):
    e = expected(case, kind)
    y, u, v = e["planes"]
    assert np.array_equal(e["packed"][..., 0], y)
    assert np.array_equal(e["packed"][..., 1], up_closed_form(u)) and np.array_equal(e["packed"][..., 2], up_closed_form(v))
    pu, pv = up_both_planes_at_once(u, v)
    assert np.array_equal(e["packed"][..., 1], pu) and np.array_equal(e["packed"][..., 2], pv)


def test_the_two_halves_never_meet_at_the_extreme_samples():
    for a, b in [(255, 255), (255, 0), (0, 255), (0, 0)]:
        u, v = np.full((3, 3), a, np.uint8), np.full((3, 3), b, np.uint8)
        pu, pv = up_both_planes_at_once(u, v)
        assert (pu == a).all() and (pv == b).all()


def fraction(a, b):
    return float((a != b).mean())


@pytest.mark.parametrize("kind", TEXTURES)
@pytest.mark.parametrize("case", [c for c in CASES if c[4] == 0.8 and c[2] >= 6 and c[3] >= 10], ids=case_id)
def test_the_sharpening_changes_every_plane(case, kind):
    e = expected(case, kind)
    plain, _, _ = chain(e["planes"], case[2], case[3], case[4], sharpen=False)
    changed = [fraction(w, p) for w, p in zip(e["want"], plain)]
    print(case_id(case), kind, "Y %.2f U %.2f V %.2f" % tuple(changed))
    assert min(changed) >= 0.25, changed


@pytest.mark.parametrize("kind", TEXTURES)
def test_the_smallest_frames(kind):
    # 2 x 2 -> 4 x 4: the luma differs from the unsharpened chain's in exactly the 2 x 2 interior
    e = expected(C_4x4, kind)
    plain, _, _ = chain(e["planes"], 4, 4, 0.8, sharpen=False)
    interior = np.zeros((4, 4), bool); interior[1:3, 1:3] = True
    assert np.array_equal(e["want"][0] != plain[0], interior)
    # 2 x 2 -> 2 x 2 is all border: the ingest -> egress round trip
    e = expected(C_2x2, kind)
    trip = oracle().egress_yuv420(e["packed"])
    assert all(np.array_equal(w, t) for w, t in zip(e["want"], trip))


@pytest.mark.parametrize("kind", TEXTURES)
@pytest.mark.parametrize("case", [c for c in CASES if c[0] >= 10 and c[1] >= 18 and not equal_sizes(c)], ids=case_id)
def test_the_upscale_is_no_nearest_neighbour_copy_and_runs_the_yuv_program(case, kind):
    e = expected(case, kind)
    rows, cols, drows, dcols, _ = case
    nearest = e["packed"][np.arange(drows) * rows // drows][:, np.arange(dcols) * cols // dcols]
    moved = float((e["scaled"] != nearest).any(axis=2).mean())
    print(case_id(case), kind, "%.2f" % moved)
    assert moved >= 0.30
    assert not np.array_equal(oracle().upscale(e["packed"], (dcols, drows), yuv=False), e["scaled"])


@pytest.mark.parametrize("kind", TEXTURES)
@pytest.mark.parametrize("ends", SHARPNESS_ENDS, ids=lambda p: case_id(p[0]))
def test_the_ends_of_the_sharpness_range_differ(ends, kind):
    lo, hi = expected(ends[0], kind), expected(ends[1], kind)
    assert ends[0][:4] == ends[1][:4] and (ends[0][4], ends[1][4]) == (0.0, 1.0)
    differ = [fraction(a, b) for a, b in zip(lo["want"], hi["want"])]
    print(case_id(ends[0]), kind, differ)
    assert min(differ) >= 0.31


@pytest.mark.parametrize("kind", TEXTURES)
def test_the_smallest_upscale_differs_between_the_ends_only_in_its_interior(kind):
    planes = expected(C_4x4, kind)["planes"]
    lo, hi = chain(planes, 4, 4, 0.0)[0], chain(planes, 4, 4, 1.0)[0]
    differ = lo[0] != hi[0]
    assert differ[1:3, 1:3].any() and int(differ.sum()) == int(differ[1:3, 1:3].sum())
    assert np.array_equal(lo[1], hi[1]) and np.array_equal(lo[2], hi[2])


@pytest.mark.parametrize("kind", TEXTURES)
@pytest.mark.parametrize("case", [c for c in CASES if equal_sizes(c) and c != C_2x2], ids=case_id)
def test_chroma_at_equal_sizes_is_not_a_copy_of_the_input(case, kind):
    # (2 x 2 has one chroma sample per plane, whose up-sampling and average are the sample itself: test_the_smallest_frames)
    e = expected(case, kind)
    assert not np.array_equal(e["want"][1], e["planes"][1]) and not np.array_equal(e["want"][2], e["planes"][2])
