"""CPU side of the lens filter object and lvk_hip_remap_map_yuv420: the surface of the nine symbols, and the conditions under which
a pass of the GPU tests (tests/test_lens_420_gpu.py) means something -- the cases of tests/lens_420_cases.py are live.  These are conditions on the cases,
not tolerances on the code; the thresholds sit below the smallest values seen with the two textures at seed 11:
  * primitive cases of 16 x 34 and larger: the near, far and lens maps together put pixels in every class of the kernel (EASU, border copy, background);
    smallest counts seen, at 16 x 34: 649 / 416 / 567 of 1632 -- asserted > 0 each;
  * filter cases of 66 rows and more with a profile: the fraction of bytes that differ from the plain ingest -> egress round trip is at least 0.715 in
    every plane (asserted >= 0.65); without a profile the planes ARE the round trip;
  * filter cases of 66 rows and more: the test-mode planes differ from the others in at least 0.431 of the bytes of every plane (asserted >= 0.40);
  * profile 3 has no distortion, but its view region is one row and one column short of the frame, so crop_in moves it: not the round trip either."""
import os
import re

import numpy as np
import pytest

from tests.lens_420_cases import (FILTER_PROFILES, FILTER_SIZES, PRIM_SIZES, SEQUENCE_SIZES, TEXTURES, classify, filter_expected, offset_map, profile_id,
                                  size_id)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["lvk_hip_remap_map_yuv420", "lvk_hip_lens_create", "lvk_hip_lens_configure", "lvk_hip_lens_destroy", "lvk_hip_lens_view", "lvk_hip_lens_apply",
         "lvk_hip_lens_apply_gray", "lvk_hip_lens_apply_c4", "lvk_hip_lens_apply_yuv420"]
ARITY = {"lvk_hip_remap_map_yuv420": 15, "lvk_hip_lens_create": 4, "lvk_hip_lens_configure": 3, "lvk_hip_lens_destroy": 1, "lvk_hip_lens_view": 4,
         "lvk_hip_lens_apply": 8, "lvk_hip_lens_apply_gray": 7, "lvk_hip_lens_apply_c4": 8, "lvk_hip_lens_apply_yuv420": 16}


def header():
    return open(os.path.join(ROOT, "include", "lvk_hip.h")).read()


def test_the_nine_symbols_are_declared_in_part_2_bound_and_exported():
    import ctypes
    from livevisionkit_amd import _native
    text = header()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    stable = re.sub(r"/\*.*?\*/", "", stable, flags=re.S)
    # inside lvk_hip.h itself, above the closing `#ifdef __cplusplus`: the header's tail keeps exactly its three includes
    body = re.sub(r"/\*.*?\*/", "", experimental[:experimental.rindex("#ifdef __cplusplus")], flags=re.S)
    lib = _native.load()
    for name in NAMES:
        decl = re.search(r"^(?:int|void)\s+%s\((.*?)\);" % name, body, re.S | re.M)
        assert decl, name
        assert not re.search(r"\b%s\s*\(" % name, stable), name
        assert len(decl.group(1).split(",")) == ARITY[name], name
        assert name in _native.symbols()
        fn = getattr(lib, name)
        assert len(fn.argtypes) == ARITY[name], name
        assert fn.restype is (None if name == "lvk_hip_lens_destroy" else ctypes.c_int)
    assert "typedef struct lvk_hip_lens lvk_hip_lens;" in body
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integration for n in NAMES) and "LCFilter" in integration


def test_a_null_context_or_object_is_refused():
    import ctypes
    from livevisionkit_amd import _native
    lib = _native.load()
    out = ctypes.c_void_p()
    view = (ctypes.c_int * 4)()
    bg = (ctypes.c_uint8 * 3)(0, 0, 0)
    assert lib.lvk_hip_lens_create(None, None, 0, ctypes.byref(out)) == -1 and not out.value
    assert lib.lvk_hip_remap_map_yuv420(None, None, 0, 0, 0, None, 0, None, 0, None, 0, 0, None, 0, bg) == -1
    assert lib.lvk_hip_lens_configure(None, None, 0) == -1
    assert lib.lvk_hip_lens_view(None, 8, 8, view) == -1
    assert lib.lvk_hip_lens_apply(None, None, 0, 0, 0, 0, None, 0) == -1
    assert lib.lvk_hip_lens_apply_gray(None, None, 0, 0, 0, None, 0) == -1
    assert lib.lvk_hip_lens_apply_c4(None, None, 0, 0, 0, 1, None, 0) == -1
    assert lib.lvk_hip_lens_apply_yuv420(None, *([None, 0] * 6), 0, 0, 0) == -1
    lib.lvk_hip_lens_destroy(None)


def test_the_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "lens.c"
    src.write_text('#include "lvk_hip.h"\nint main(void) { lvk_hip_lens* l = 0; (void)l; %s return 0; }\n' % " ".join("(void)%s;" % n for n in NAMES))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_the_python_names_exist():
    import livevisionkit_amd as lvk
    assert "LCFilter" in lvk.__all__ and callable(lvk.Context.remap_map_yuv420)
    for m in ("configure", "apply", "apply_yuv420", "view", "close"):
        assert callable(getattr(lvk.LCFilter, m)), m
    facade = open(os.path.join(ROOT, "include", "lvk", "LiveVisionKit.hpp")).read()
    assert '#include "LCFilter.hpp"' in facade


@pytest.mark.parametrize("size", [s for s in PRIM_SIZES if s[0] >= 16 and s[1] >= 34], ids=size_id)
def test_the_three_maps_reach_every_class_of_the_kernel(size):
    rows, cols = size
    counts = np.zeros(3, np.int64)
    for name in ("near", "far", "lens"):
        counts += np.bincount(classify(offset_map(name, rows, cols), rows, cols).ravel(), minlength=3)
    print(size_id(size), "EASU %d border %d background %d" % tuple(counts))
    assert (counts > 0).all(), counts


def test_the_smallest_frames_have_no_interior():
    # 2 x 2 and 4 x 6: 1 <= sy < rows - 4 leaves no pixel for EASU: all border copy or background.  6 x 8 has one source row (sy = 1, sx = 1 .. 3)
    # that EASU can start from: its interior is that sliver, and the near map reaches it.
    for size in [(2, 2), (4, 6)]:
        for name in ("near", "far", "nonfinite"):
            assert not (classify(offset_map(name, *size), *size) == 0).any(), (size, name)
    c = classify(offset_map("near", 6, 8), 6, 8)
    assert 0 < int((c == 0).sum()) <= 6 and (c == 1).any() and (c == 2).any()


def test_non_finite_offsets_take_the_paths_of_the_conversion():
    m = np.zeros((8, 12, 2), np.float32)
    m[2, 3] = (np.nan, 0); m[3, 3] = (np.inf, 0); m[4, 4] = (-np.inf, 0); m[5, 5] = (1e30, -1e30)
    c = classify(m, 8, 12)
    assert c[2, 3] == 1            # NaN -> column 0: a border copy
    assert c[3, 3] == 2 and c[4, 4] == 2 and c[5, 5] == 2


def fractions(a, b):
    return [float((x != y).mean()) for x, y in zip(a, b)]


LARGE = [s for s in FILTER_SIZES + SEQUENCE_SIZES if s[0] >= 66]


@pytest.mark.parametrize("kind", TEXTURES)
@pytest.mark.parametrize("profile", FILTER_PROFILES, ids=profile_id)
@pytest.mark.parametrize("size", LARGE, ids=size_id)
def test_the_correction_changes_the_planes_and_no_profile_is_the_round_trip(size, profile, kind):
    e = filter_expected(size, profile, False, kind)
    moved = fractions(e["want"], e["round_trip"])
    print(size_id(size), profile_id(profile), kind, "Y %.3f U %.3f V %.3f" % tuple(moved))
    if profile is None:
        assert max(moved) == 0.0 and e["view"] == (0, 0, size[1], size[0])
        # ... which is not a copy of the input chroma: it went up and down again
        assert not np.array_equal(e["want"][1], e["planes"][1]) and np.array_equal(e["want"][0], e["planes"][0])
    else:
        assert min(moved) >= 0.65, moved


@pytest.mark.parametrize("kind", TEXTURES)
@pytest.mark.parametrize("profile", FILTER_PROFILES, ids=profile_id)
@pytest.mark.parametrize("size", LARGE, ids=size_id)
def test_the_test_mode_changes_the_planes(size, profile, kind):
    off, on = filter_expected(size, profile, False, kind), filter_expected(size, profile, True, kind)
    differ = fractions(off["want"], on["want"])
    print(size_id(size), profile_id(profile), kind, "Y %.3f U %.3f V %.3f" % tuple(differ))
    assert min(differ) >= 0.40, differ


@pytest.mark.parametrize("size", LARGE, ids=size_id)
def test_profile_3_moves_the_view_although_it_has_no_distortion(size):
    for kind in TEXTURES:
        e = filter_expected(size, 3, False, kind)
        x, y, w, h = e["view"]
        assert (x, y, w, h) != (0, 0, size[1], size[0]) and w > 0 and h > 0
        assert all(not np.array_equal(a, b) for a, b in zip(e["want"], e["round_trip"]))
