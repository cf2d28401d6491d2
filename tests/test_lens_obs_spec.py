"""CPU side of lvk_hip_remap_map_obs and lvk_hip_lens_apply_obs: the surface of the two symbols, the specification of
tests/lens_obs_cases.py against the one the 4:2:0 tests already use, and the conditions under which a pass of tests/test_lens_obs_gpu.py means something
-- no test there can pass on a pass-through.  These are conditions on the cases, not tolerances on the code:
  * profiles 0 and 1: at least 0.4 of every output plane's bytes differ from the no-profile round trip, over every filter size (odd ones included), all
    sixteen formats and both textures; the smallest shares seen are 0.496 (AYUV, whose alpha byte never changes) and 0.502 (9 x 13 RGBA, where a quarter
    of the plane is never written);
  * with the grid on at least 0.3 of every plane's bytes differ from the same case without it; smallest seen 0.325 (270 x 480, AYUV and the 4-byte formats);
  * every `far` map of a primitive size from 66 x 254 up puts pixels in all three classes of the kernel (EASU, border copy, background)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import lens_420_cases as c420
from tests.lens_obs_cases import (DIRECT4, FILTER_PROFILES, FORMATS, PRIM_SIZES_422, PRIM_SIZES_444, TEXTURES, chain, classify, filter_expected, filter_sizes,
                                  offset_map, plane_shapes, prim_expected, profile_id, size_id, written_mask)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"lvk_hip_remap_map_obs": 11, "lvk_hip_lens_apply_obs": 8}


def test_the_two_symbols_are_declared_in_part_2_bound_and_exported():
    from livevisionkit_amd import _native
    text = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    stable = re.sub(r"/\*.*?\*/", "", stable, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", experimental[:experimental.rindex("#ifdef __cplusplus")], flags=re.S)
    lib = _native.load()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, arity in ARITY.items():
        decl = re.search(r"^int\s+%s\((.*?)\);" % name, body, re.S | re.M)
        assert decl, name
        assert not re.search(r"\b%s\s*\(" % name, stable), name
        assert len(decl.group(1).split(",")) == arity, name
        assert name in _native.symbols()
        fn = getattr(lib, name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
        assert name in integration, name
    # no ABI bump: PART 1 is what it was
    assert re.search(r"#define LVK_HIP_ABI_VERSION 12\b", text)


def test_a_null_context_or_object_is_refused():
    from livevisionkit_amd import _native
    lib = _native.load()
    ptrs, steps = (ctypes.c_void_p * 3)(), (ctypes.c_int * 3)()
    bg = (ctypes.c_uint8 * 3)(0, 0, 0)
    assert lib.lvk_hip_remap_map_obs(None, 5, None, 0, 8, 8, ptrs, steps, None, 0, bg) == -1
    assert lib.lvk_hip_lens_apply_obs(None, 5, ptrs, steps, ptrs, steps, 8, 8) == -1


def test_the_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "lens_obs.c"
    src.write_text('#include "lvk_hip.h"\nint main(void) { %s return 0; }\n' % " ".join("(void)%s;" % n for n in ARITY))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_the_python_names_exist():
    import livevisionkit_amd as lvk
    assert callable(lvk.Context.remap_map_obs) and callable(lvk.LCFilter.apply_obs)
    assert lvk.LCFilter.obs_plane_shapes("Y800", 4, 6) == [(4, 6)]
    for fmt in FORMATS:
        assert [tuple(s) for s in lvk.LCFilter.obs_plane_shapes(fmt, 8, 10)] == [tuple(s) for s in plane_shapes(fmt, 8, 10)], fmt
    facade = open(os.path.join(ROOT, "include", "lvk", "LiveVisionKit.hpp")).read()
    assert "struct VideoFrameOBS" in facade


@pytest.mark.parametrize("test_mode", [False, True], ids=["plain", "grid"])
@pytest.mark.parametrize("profile", FILTER_PROFILES, ids=profile_id)
@pytest.mark.parametrize("size", [(16, 34), (66, 258)], ids=size_id)
def test_the_specification_of_the_420_formats_is_the_one_of_the_420_entry(size, profile, test_mode):
    for kind in TEXTURES:
        e = c420.filter_expected(size, profile, test_mode, kind)
        for fmt, lay in (("I420", tuple), ("I40A", tuple), ("NV12", c420.as_nv12)):
            got, view = chain(fmt, lay(e["planes"]), profile, test_mode)
            assert view == e["view"]
            for g, w in zip(got, lay(e["want"])):
                assert np.array_equal(g, w), (fmt, kind)


def test_the_packed_422_expectations_are_byte_permutations_of_one_another():
    for size in [(9, 18), (66, 258)]:
        for name in ("near", "far"):
            yuy2, yvyu, uyvy = (prim_expected(f, size, name, "random")["want"][0] for f in ("YUY2", "YVYU", "UYVY"))
            y, u, v = prim_expected("I422", size, name, "random")["want"]
            # [rows, cols, 2] viewed as [rows, cols / 2, 4]: Y0 U Y1 V | Y0 V Y1 U | U Y0 V Y1
            a, b, c = (p.reshape(size[0], size[1] // 2, 4) for p in (yuy2, yvyu, uyvy))
            assert np.array_equal(a[..., [0, 3, 2, 1]], b) and np.array_equal(a[..., [1, 0, 3, 2]], c)
            assert np.array_equal(a[..., [0, 2]].reshape(size), y) and np.array_equal(a[..., 1], u) and np.array_equal(a[..., 3], v)
            assert not np.array_equal(u, v)


def fractions(a, b):
    return [float((x != y).mean()) for x, y in zip(a, b)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_correction_changes_every_plane_and_no_profile_is_the_round_trip(fmt):
    low = 1.0
    for size in filter_sizes(fmt):
        for kind in TEXTURES:
            none = filter_expected(fmt, size, None, False, kind)
            assert all(np.array_equal(a, b) for a, b in zip(none["want"], none["round_trip"])) and none["view"] == (0, 0, size[1], size[0])
            for profile in (0, 1):
                e = filter_expected(fmt, size, profile, False, kind)
                moved = fractions(e["want"], e["round_trip"])
                low = min(low, *moved)
                assert min(moved) >= 0.4, (size, profile, kind, moved)
            # profile 3 has no distortion, but its view region moves the frame: not the round trip either
            e3 = filter_expected(fmt, size, 3, False, kind)
            assert size[0] < 16 or all(not np.array_equal(a, b) for a, b in zip(e3["want"], e3["round_trip"])), (size, kind)
    print(fmt, "smallest share of bytes a profile moves: %.3f" % low)


@pytest.mark.parametrize("fmt", [f for f in FORMATS if f != "Y800"])
def test_the_test_mode_changes_every_plane(fmt):
    low = 1.0
    for size in filter_sizes(fmt):
        for profile in FILTER_PROFILES:
            for kind in TEXTURES:
                off, on = filter_expected(fmt, size, profile, False, kind), filter_expected(fmt, size, profile, True, kind)
                differ = fractions(off["want"], on["want"])
                low = min(low, *differ)
                assert min(differ) >= 0.3, (size, profile, kind, differ)
    print(fmt, "smallest share of bytes the grid changes: %.3f" % low)


def test_the_subsampled_round_trip_is_not_a_copy_of_the_input_chroma():
    for fmt in ("I422", "UYVY", "I420"):
        e = filter_expected(fmt, (66, 258), None, False, "random")
        assert not all(np.array_equal(a, b) for a, b in zip(e["want"], e["planes"])), fmt
    for fmt in ("I444", "AYUV", "BGR3", "Y800"):
        e = filter_expected(fmt, (66, 258), None, False, "random")
        assert all(np.array_equal(a, b) for a, b in zip(e["want"], e["planes"])), fmt


def test_the_direct_formats_leave_the_last_quarter_alone():
    for fmt in DIRECT4:
        e = filter_expected(fmt, (9, 13), 0, False, "random")
        mask = written_mask(fmt, 9, 13)[0]
        assert (e["want"][0][~mask] == 0x5A).all() and abs(float(mask.mean()) - 0.75) < 1e-9
        assert not (e["want"][0][mask] == 0x5A).all()


@pytest.mark.parametrize("size", sorted({s for s in PRIM_SIZES_422 + PRIM_SIZES_444 if s[0] >= 66}), ids=size_id)
def test_every_far_map_reaches_every_class_of_the_kernel(size):
    counts = np.bincount(classify(offset_map("far", *size), *size).ravel(), minlength=3)
    print(size_id(size), "EASU %d border %d background %d" % tuple(counts))
    assert (counts > 0).all(), counts
