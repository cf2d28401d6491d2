"""CPU side of lvk_hip_cas_yuv420 / lvk_hip_cas_obs: the symbols' surface, and the conditions under which a pass of the GPU tests
(tests/test_cas_obs_gpu.py) means something -- the luma out is the one-channel filter of the luma in; each plane of I444 is the one-channel filter of that
plane; at 2 x 2 the expected chroma equals a hand-written evaluation in which the replicated up-sampling meets the zero border of CAS; the filter changes
the planes (a byte-identical round trip would pass a copy kernel); and the sharpness is used."""
import os
import re

import numpy as np
import pytest

from tests import np_cas as nc
from tests.cas_obs_cases import (CASES, F420, F422, FORMATS, FRAME_YUV, FULL_CASES, GUARD, SHARPNESS, SIZES_420, SIZES_422, SIZES_ODD, case_id, changed_shares,
                                 expected, sizes_of, written_mask)
from tests.ffx_gray_cases import cas_gray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARGS_420 = ["const void* d_y", "int y_step", "const void* d_u", "int u_step", "const void* d_v", "int v_step",
            "void* o_y", "int oy_step", "void* o_u", "int ou_step", "void* o_v", "int ov_step", "int rows", "int cols", "int nv12", "float sharpness"]
ARGS_OBS = ["int video_format", "const void* const d_planes[3]", "const int steps[3]", "void* const o_planes[3]", "const int o_steps[3]",
            "int rows", "int cols", "float sharpness"]


def test_symbols_are_declared_bound_and_exported():
    """include/lvk_hip_cas_obs.h declares exactly the two entries, lvk_hip.h reaches it in its PART 2 through lvk_hip_deblock_420.h and
    lvk_hip_deblock_obs.h (inside the include guards), and livevisionkit_amd/_native.py binds exactly what it declares."""
    import ctypes
    from livevisionkit_amd import _native
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvk_hip_cas_obs.h")).read(), flags=re.S)
    assert sorted(re.findall(r"\b(lvk_(?:hip|stab)_[a-z0-9_]+)\s*\(", code)) == ["lvk_hip_cas_obs", "lvk_hip_cas_yuv420"] == _native.symbols_cas_obs()
    for name, args in (("lvk_hip_cas_yuv420", ARGS_420), ("lvk_hip_cas_obs", ARGS_OBS)):
        decl = re.search(r"^int %s\(lvk_hip_ctx\* ctx,(.*?)\);" % name, code, re.S | re.M)
        assert decl and [a.strip() for a in decl.group(1).replace("\n", " ").split(",")] == args, name
        fn = getattr(_native.load(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 1 + len(args)
    hobs = open(os.path.join(ROOT, "include", "lvk_hip_deblock_obs.h")).read()
    assert re.search(r'^#include "lvk_hip_cas_obs.h"', hobs, re.M) and hobs.rstrip().endswith("#endif /* LVK_HIP_DEBLOCK_OBS_H */")
    text = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    stable, _ = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    assert "lvk_hip_cas_obs" not in stable and "lvk_hip_cas_yuv420" not in stable
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "lvk_hip_cas_obs" in integration and "lvk_hip_cas_yuv420" in integration
    lib = _native.load()
    none3, zero3 = (ctypes.c_void_p * 3)(), (ctypes.c_int * 3)()
    assert lib.lvk_hip_cas_obs(None, 1, none3, zero3, none3, zero3, 0, 0, 0.5) != 0       # a NULL context is refused before anything is touched
    assert lib.lvk_hip_cas_yuv420(None, *([None, 0] * 6), 0, 0, 0, 0.5) != 0
    import livevisionkit_amd as lvk
    assert callable(lvk.CASFilter.apply_obs) and callable(lvk.CASFilter.apply_yuv420)


def test_the_header_is_plain_c_whichever_header_comes_first(tmp_path):
    """C99 with -pedantic: alone, and before or after lvk_hip.h and the headers that include it."""
    import subprocess
    for heads in (("lvk_hip_cas_obs.h",), ("lvk_hip.h", "lvk_hip_cas_obs.h"), ("lvk_hip_cas_obs.h", "lvk_hip.h"), ("lvk_hip_deblock_obs.h",),
                  ("lvk_hip_cas_obs.h", "lvk_hip_deblock_420.h"), ("lvk_hip.h",)):
        src = tmp_path / "cobs.c"
        src.write_text("".join('#include "%s"\n' % h for h in heads)
                       + 'int main(void) { (void)lvk_hip_cas_obs; (void)lvk_hip_cas_yuv420; (void)lvk_hip_cas; (void)lvk_hip_deblock_apply_obs; return 0; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_the_makefile_rule_lists_the_new_header_and_the_units_are_sources():
    text = open(os.path.join(ROOT, "livevisionkit_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^%\.o: %\.hip (.*)$", text, re.M).group(1).split()
    for h in ("cas_core.hpp", "yuv420_core.hpp", "obs_planes.hpp", "obs_sinks.hpp", "../../include/lvk_hip_cas_obs.h"):
        assert h in rule, h
    assert re.search(r"^SRCS = \$\(wildcard \*\.hip\)$", text, re.M)
    for unit in ("cas_420.hip", "cas_obs.hip"):
        assert os.path.exists(os.path.join(ROOT, "livevisionkit_amd", "csrc", unit))


def test_the_case_list_is_the_one_the_tests_mean():
    assert len(FORMATS) == 16 and len(CASES) == sum(len(sizes_of(f)) for f in FORMATS) == 3 * 8 + 5 * 7 + 8 * 11
    assert SIZES_420 == [(2, 2), (4, 6), (6, 10), (8, 14), (18, 34), (66, 254), (66, 256), (68, 258)]
    assert SIZES_422 == [(2, 2), (3, 6), (9, 14), (17, 34), (66, 254), (66, 256), (67, 258)]
    assert SIZES_ODD == [(3, 5), (9, 13), (17, 35), (67, 257)] and SHARPNESS == [0.0, 0.8, 1.0]
    assert all(s[1] % 2 == 0 for f, s in CASES if f in F422) and all((s[0] | s[1]) % 2 == 0 for f, s in CASES if f in F420)
    assert sorted(f for f, _ in FULL_CASES) == ["I420", "UYVY"] and all(s == (1080, 1920) for _, s in FULL_CASES)


def luma_of(fmt, planes):
    """The luma samples [rows, cols] of the planes of a YUV format"""
    if fmt in ("YUY2", "YVYU"):
        return planes[0][..., 0]
    if fmt == "UYVY":
        return planes[0][..., 1]
    if fmt == "AYUV":
        return planes[0][..., 1]
    return planes[0]


@pytest.mark.parametrize("fc", [fc for fc in CASES if fc[0] in FRAME_YUV], ids=case_id)
def test_the_luma_out_is_the_gray_filter_of_the_luma_in(fc):
    fmt, size = fc
    for s in SHARPNESS:
        e = expected(fmt, size, s)
        assert np.array_equal(luma_of(fmt, e["want"]), cas_gray(np.ascontiguousarray(luma_of(fmt, e["planes"])), s)), s


@pytest.mark.parametrize("size", sizes_of("I444"), ids=lambda s: "%dx%d" % s)
def test_every_plane_of_i444_is_the_gray_filter_of_that_plane(size):
    for s in SHARPNESS:
        e = expected("I444", size, s)
        for i in range(3):
            assert np.array_equal(e["want"][i], cas_gray(e["planes"][i], s)), (s, i)


def cas_pixel(pad, y, x, peak):
    """CasFilter for the pixel whose 3 x 3 window starts at pad[y, x], one scalar operation after the other (float32, each rounded on its own)"""
    f32 = np.float32
    a, b, c, d, e, f, g, h, i = (f32(v) for v in pad[y:y + 3, x:x + 3].reshape(-1))
    mn = min(d, e, f, b, h)
    mn = f32(mn + min(mn, a, c, g, i))
    mx = max(d, e, f, b, h)
    mx = f32(mx + max(mx, a, c, g, i))
    amp = nc.lo_sqrt(nc.sat(f32(min(mn, f32(f32(2) - mx)) * nc.lo_rcp(mx))))
    w = f32(amp * f32(peak))
    total = f32(f32(f32(f32(b * w) + f32(d * w)) + f32(f * w)) + f32(h * w)) + e
    return float(nc.sat(f32(f32(total) * nc.med_rcp(f32(f32(1) + f32(f32(4) * w))))))


@pytest.mark.parametrize("fmt", F420)
def test_the_two_edge_rules_at_2x2(fmt):
    """One chroma sample per plane: the ingest replicates it over the 2 x 2 frame, CAS reads zeros around the frame (not the replicated value), and the
    egress takes the 2 x 2 mean (sum + 2) >> 2 of the four sharpened values."""
    for s in SHARPNESS:
        e = expected(fmt, (2, 2), s)
        peak = nc.peak_of(s)
        for ch in (0, 1):
            sample = int(e["planes"][1][0, 0, ch] if fmt == "NV12" else e["planes"][1 + ch][0, 0])
            pad = np.zeros((4, 4), np.float32)
            pad[1:3, 1:3] = nc.UNIT[sample]                    # the up-sampled value everywhere, zeros around it
            out = [int(np.rint(np.float32(cas_pixel(pad, y, x, peak)) * np.float32(255))) for y in range(2) for x in range(2)]
            mean = (sum(out) + 2) >> 2
            got = int(e["want"][1][0, 0, ch] if fmt == "NV12" else e["want"][1 + ch][0, 0])
            assert got == mean, (s, ch, sample, out)


@pytest.mark.parametrize("fc", CASES, ids=case_id)
def test_the_filter_changes_the_planes(fc):
    """Liveness, against the plain ingest -> egress round trip.  With rows >= 8 every written plane differs in at least half of its written bytes -- on
    the seeded noise the CPU oracle gives 0.57 to 0.96 over all formats and the three sharpness values, the lowest AYUV's, whose constant alpha byte
    counts; 0.5 is a cap against a dead test, not a tolerance.  A smaller case differs in at least one byte of the frame."""
    fmt, size = fc
    for s in SHARPNESS:
        shares = changed_shares(fmt, size, s)
        print(case_id(fc), s, " ".join("%.3f" % v for v in shares))
        if size[0] >= 8:
            assert min(shares) >= 0.5, (s, shares)
        else:
            assert max(shares) > 0.0, (s, shares)


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_sharpness_is_used(fmt):
    for size in sizes_of(fmt):
        if size[0] * size[1] < 17 * 34:
            continue
        a, b = expected(fmt, size, 0.0)["want"], expected(fmt, size, 1.0)["want"]
        assert all(not np.array_equal(x, y) for x, y in zip(a, b)), size


@pytest.mark.parametrize("fmt", FORMATS)
def test_guard_survives_exactly_where_the_egress_writes_nothing(fmt):
    size = sizes_of(fmt)[3]
    masks = written_mask(fmt, *size)
    e = expected(fmt, size, 0.8)
    for m, w in zip(masks, e["want"]):
        assert np.all(w[~m] == GUARD)
