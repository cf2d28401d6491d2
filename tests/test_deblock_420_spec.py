"""CPU side of lvk_hip_deblock_apply_yuv420: the symbol's surface, and the conditions under which a pass of the GPU tests
(tests/test_deblock_420_gpu.py) means something -- the cases of tests/deblock_420_cases.py are live: the deblocking changes the planes, the plain
ingest -> egress round trip changes the chroma, and chroma outside the filter region is not a copy of the input."""
import os
import re

import numpy as np
import pytest

from tests import np_deblock as nd
from tests.deblock_420_cases import CASES, NOT_LIVE, as_nv12, case_id, expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE = [c for c in CASES if c[:2] not in NOT_LIVE]


ARGS = ["const void* d_y", "int y_step", "const void* d_u", "int u_step", "const void* d_v", "int v_step",
        "void* o_y", "int oy_step", "void* o_u", "int ou_step", "void* o_v", "int ov_step", "int nv12", "int rows", "int cols", "int region_xywh[4]"]


def test_symbol_is_declared_bound_and_exported():
    """include/lvk_hip_deblock_420.h declares exactly the entry, lvk_hip.h includes it in its PART 2 (inside its include guard, behind its own
    declarations, as it includes lvk_hip_deblock_px.h), and livevisionkit_amd/_native.py binds exactly what it declares."""
    import ctypes
    from livevisionkit_amd import _native
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvk_hip_deblock_420.h")).read(), flags=re.S)
    assert re.findall(r"\b(lvk_(?:hip|stab)_[a-z0-9_]+)\s*\(", code) == ["lvk_hip_deblock_apply_yuv420"] == _native.symbols_deblock_420()
    decl = re.search(r"^int lvk_hip_deblock_apply_yuv420\(lvk_hip_deblock\* deb,(.*?)\);", code, re.S | re.M)
    assert decl and [a.strip() for a in decl.group(1).replace("\n", " ").split(",")] == ARGS
    stable, experimental = open(os.path.join(ROOT, "include", "lvk_hip.h")).read().split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    assert re.search(r'^#include "lvk_hip_deblock_420.h"', experimental, re.M) and "lvk_hip_deblock_420.h" not in stable
    assert "lvk_hip_deblock_apply_yuv420" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fn = _native.load().lvk_hip_deblock_apply_yuv420
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 1 + len(ARGS)
    assert fn(None, *([None, 0] * 6), 0, 0, 0, None) != 0              # a NULL handle is refused before anything is touched
    import livevisionkit_amd as lvk
    assert callable(lvk.DeblockingFilter.apply_yuv420)


def test_the_header_is_plain_c_either_way_round(tmp_path):
    """C99 with -pedantic, whichever of the two headers a host includes first."""
    import subprocess
    for first, second in (("lvk_hip.h", "lvk_hip_deblock_420.h"), ("lvk_hip_deblock_420.h", "lvk_hip.h")):
        src = tmp_path / "d420.c"
        src.write_text('#include "%s"\n#include "%s"\n'
                       'int main(void) { (void)lvk_hip_deblock_apply_yuv420; (void)lvk_hip_deblock_apply; return 0; }\n' % (first, second))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_ingest_of_i420_and_of_the_same_samples_as_nv12_agree(oracle, case):
    e = expected(case)
    assert np.array_equal(oracle.ingest_yuv420(*as_nv12(e["planes"])), e["packed"])
    y, uv = oracle.egress_yuv420(e["packed"], nv12=True)
    assert np.array_equal(y, e["trip"][0]) and np.array_equal(uv[..., 0], e["trip"][1]) and np.array_equal(uv[..., 1], e["trip"][2])


@pytest.mark.parametrize("case", LIVE, ids=case_id)
def test_cases_are_live(case):
    e = expected(case)
    for i, (want, trip, src) in enumerate(zip(e["want"], e["trip"], e["planes"])):
        changed = int((want != trip).sum())
        assert changed * 5 >= want.size, (i, changed, want.size)           # what the deblocking itself does (lowest of the issue's table: 32 %)
        if i:
            moved = int((trip != src).sum())
            assert moved * 2 >= src.size, (i, moved, src.size)             # the round trip is no copy of the chroma (lowest measured: 69 %)


@pytest.mark.parametrize("case", NOT_LIVE)
def test_one_block_frames_are_not_live(case):
    e = expected([c for c in CASES if c[:2] == case][0])
    assert all(np.array_equal(w, t) for w, t in zip(e["want"], e["trip"]))


def outside_quads(case):
    """Chroma samples whose 2 x 2 quad lies wholly outside the filter region: (how many, how many of them differ from the input) summed over U and V."""
    e = expected(case)
    _, _, RW, RH = e["info"]["region"]
    rows, cols = case[:2]
    cy, cx = np.mgrid[0:rows // 2, 0:cols // 2]
    outside = (2 * cx >= RW) | (2 * cy >= RH)
    n = 2 * int(outside.sum())
    differ = sum(int((e["want"][i][outside] != e["planes"][i][outside]).sum()) for i in (1, 2))
    same_as_trip = all(np.array_equal(e["want"][i][outside], e["trip"][i][outside]) for i in (1, 2))
    return n, differ, same_as_trip


# The cases whose region is smaller than the frame.  Two of them (30 x 34 and 34 x 30: a region of 33 of 34 columns / rows) leave one luma column or
# row outside, so every quad there STRADDLES the edge and none lies wholly outside; the condition below is asserted for the seven others.
SMALLER = [c for c in CASES if c[0] % c[3] or c[1] % c[3]]
STRADDLING_ONLY = [(30, 34), (34, 30)]
# Chroma samples (U and V together) whose quad lies wholly outside the region and which differ from the input, of those outside:
#   50x38: 48 / 50    66x130: 181 / 194    48x86: 112 / 144    34x50: 81 / 82    70x100: 327 / 428    130x258: 375 / 386    1080x1920: 5241 / 7680
WITH_OUTSIDE = [c for c in SMALLER if c[:2] not in STRADDLING_ONLY]


@pytest.mark.parametrize("case", WITH_OUTSIDE, ids=case_id)
def test_chroma_outside_the_region_is_not_a_copy_of_the_input(case):
    n, differ, same_as_trip = outside_quads(case)
    print("%s: %d / %d" % (case_id(case), differ, n))
    assert n > 0 and differ >= 1
    assert same_as_trip                  # outside the region the output is the round trip's


def test_the_cases_with_a_smaller_region_are_the_nine_of_the_table():
    assert [c[:2] for c in SMALLER] == [(30, 34), (34, 30), (50, 38), (66, 130), (48, 86), (34, 50), (70, 100), (130, 258), (1080, 1920)]
    for case in SMALLER:
        assert (outside_quads(case)[0] == 0) == (case[:2] in STRADDLING_ONLY)


def up_closed_form(c):
    """The 2x up-sampling as csrc/deblock_420.hip restates it from the comment above k_ingest_yuv420_x2: t = 3 C[c] + C[f] horizontally,
    (((3 t_k) >> 2) + (t_g >> 2) + 2) >> 2 vertically, f / g the outer neighbour of the sample, clamped to the plane."""
    c = c.astype(np.int64)
    cr, cc = c.shape
    x, y = np.arange(2 * cc), np.arange(2 * cr)
    near_x, far_x = x // 2, np.clip(np.where(x & 1, x // 2 + 1, x // 2 - 1), 0, cc - 1)
    near_y, far_y = y // 2, np.clip(np.where(y & 1, y // 2 + 1, y // 2 - 1), 0, cr - 1)
    t = 3 * c[:, near_x] + c[:, far_x]
    return (((3 * t[near_y]) >> 2) + (t[far_y] >> 2) + 2) >> 2


@pytest.mark.parametrize("case", CASES[:-1], ids=case_id)
def test_closed_form_of_the_up_sampling_is_the_ingest(case):
    e = expected(case)
    y, u, v = e["planes"]
    assert np.array_equal(e["packed"][..., 0], y)
    assert np.array_equal(e["packed"][..., 1], up_closed_form(u)) and np.array_equal(e["packed"][..., 2], up_closed_form(v))


def test_the_yuv_grey_is_the_luma_plane():
    # the block statistics of the one call read the Y plane: np_deblock's grey of a YUV frame is channel 0, which the ingest copies from Y
    e = expected(CASES[6])
    assert np.array_equal(nd.gray_of(e["packed"], nd.FMT_YUV), e["planes"][0])
