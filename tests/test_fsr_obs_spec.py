"""CPU side of lvk_hip_fsr_yuv420 / lvk_hip_fsr_obs: the symbols' surface, and the conditions under which a pass of the GPU tests
(tests/test_fsr_obs_gpu.py) means something -- constants stay constants; the luma out depends on the chroma in; the region is used, pixel by pixel; at
2 x 2 the expected planes equal a hand-written evaluation in which every tap is clamped; the chroma the taps read has the phase of the frame, not of the
region; and every case runs on the path it was chosen for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import np_fsr as nf
from tests.fsr_obs_cases import (CASES, CROP_CASES, CROP_FORMATS, DIRECT, F420, FORMATS, FULL_CASES, GUARD, PAIRS_420, PAIRS_422, PAIRS_ODD, PATHS,
                                 SIZE_CASES, STAGED, case_id, chain, egress, expected, inputs, noise, region_of, written_mask)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

ARGS_420 = ["const void* d_y", "int y_step", "const void* d_u", "int u_step", "const void* d_v", "int v_step", "int rows", "int cols",
            "const int region_xywh[4]", "void* o_y", "int oy_step", "void* o_u", "int ou_step", "void* o_v", "int ov_step", "int out_rows", "int out_cols",
            "int nv12"]
ARGS_OBS = ["int video_format", "const void* const d_planes[3]", "const int steps[3]", "int rows", "int cols", "const int region_xywh[4]",
            "void* const o_planes[3]", "const int o_steps[3]", "int out_rows", "int out_cols"]
NAMES = ["lvk_hip_fsr_obs", "lvk_hip_fsr_obs_path", "lvk_hip_fsr_yuv420"]


def test_symbols_are_declared_bound_and_exported():
    """include/lvk_hip_fsr_obs.h declares exactly the three entries, lvk_hip.h reaches it in its PART 2 through lvk_hip_cas_obs.h (inside the include
    guards), and livevisionkit_amd/_native.py binds exactly what it declares."""
    from livevisionkit_amd import _native
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvk_hip_fsr_obs.h")).read(), flags=re.S)
    assert sorted(re.findall(r"\b(lvk_(?:hip|stab)_[a-z0-9_]+)\s*\(", code)) == NAMES == _native.symbols_fsr_obs()
    for name, args in (("lvk_hip_fsr_yuv420", ARGS_420), ("lvk_hip_fsr_obs", ARGS_OBS)):
        decl = re.search(r"^int %s\(lvk_hip_ctx\* ctx,(.*?)\);" % name, code, re.S | re.M)
        assert decl and [a.strip() for a in decl.group(1).replace("\n", " ").split(",")] == args, name
        fn = getattr(_native.load(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 1 + len(args)
    assert re.search(r"^int lvk_hip_fsr_obs_path\(int rw, int rh, int out_rows, int out_cols\);", code, re.M)
    hcas = open(os.path.join(ROOT, "include", "lvk_hip_cas_obs.h")).read()
    assert re.search(r'^#include "lvk_hip_fsr_obs.h"', hcas, re.M) and hcas.rstrip().endswith("#endif /* LVK_HIP_CAS_OBS_H */")
    text = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    assert not [n for n in NAMES if n in stable] and "lvk_hip_fsr_obs.h" not in stable
    tail = experimental[experimental.rindex("#ifdef __cplusplus"):]
    assert re.findall(r'^#include "(.*?)"', tail, re.M) == ["lvk_hip_scaling_420.h", "lvk_hip_deblock_420.h", "lvk_hip_deblock_px.h"]      # as they were
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integration for n in NAMES)
    lib = _native.load()
    none3, zero3, region = (ctypes.c_void_p * 3)(), (ctypes.c_int * 3)(), (ctypes.c_int * 4)(0, 0, 2, 2)
    assert lib.lvk_hip_fsr_obs(None, 1, none3, zero3, 2, 2, region, none3, zero3, 2, 2) != 0       # a NULL context is refused before anything is touched
    assert lib.lvk_hip_fsr_yuv420(None, *([None, 0] * 3), 2, 2, region, *([None, 0] * 3), 2, 2, 0) != 0
    import livevisionkit_amd as lvk
    assert callable(lvk.FSRFilter.apply_obs) and callable(lvk.FSRFilter.apply_yuv420)


def test_the_header_is_plain_c_whichever_header_comes_first(tmp_path):
    """C99 with -pedantic: alone, and before or after lvk_hip.h and the headers that include it."""
    for heads in (("lvk_hip_fsr_obs.h",), ("lvk_hip.h", "lvk_hip_fsr_obs.h"), ("lvk_hip_fsr_obs.h", "lvk_hip.h"), ("lvk_hip_cas_obs.h",),
                  ("lvk_hip_fsr_obs.h", "lvk_hip_cas_obs.h"), ("lvk_hip.h",)):
        src = tmp_path / "fobs.c"
        src.write_text("".join('#include "%s"\n' % h for h in heads)
                       + "int main(void) { (void)lvk_hip_fsr_obs; (void)lvk_hip_fsr_yuv420; (void)lvk_hip_fsr_obs_path; (void)lvk_hip_fsr_easu;"
                         " (void)lvk_hip_cas_obs; return 0; }\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_the_makefile_rule_lists_the_new_headers_and_the_units_are_sources():
    text = open(os.path.join(ROOT, "livevisionkit_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^%\.o: %\.hip (.*)$", text, re.M).group(1).split()
    for h in ("fsr_core.hpp", "fsr_planes.hpp", "yuv420_core.hpp", "obs_planes.hpp", "obs_sinks.hpp", "../../include/lvk_hip_fsr_obs.h"):
        assert h in rule, h
    assert re.search(r"^SRCS = \$\(wildcard \*\.hip\)$", text, re.M)
    for unit in ("fsr_420.hip", "fsr_obs.hip", "fsr_planes.hpp"):
        assert os.path.exists(os.path.join(ROOT, "livevisionkit_amd", "csrc", unit))


def test_the_case_list_is_the_one_the_tests_mean():
    assert len(FORMATS) == 16 and len(SIZE_CASES) == 16 * 12 and len(CROP_CASES) == 9 * 6 and len(CASES) == len(SIZE_CASES) + len(CROP_CASES)
    assert [p[:2] for p in PAIRS_ODD] == [((2, 2), (2, 2)), ((2, 2), (4, 4)), ((3, 5), (5, 9)), ((10, 18), (15, 63)), ((10, 18), (16, 64)),
                                          ((10, 18), (17, 65)), ((24, 40), (34, 62)), ((24, 40), (18, 30)), ((48, 96), (34, 66)), ((40, 80), (16, 64)),
                                          ((40, 80), (17, 65)), ((66, 130), (34, 66))]
    assert all(s[1] % 2 == 0 and d[1] % 2 == 0 for s, d, _ in PAIRS_422) and all((s[0] | s[1] | d[0] | d[1]) % 2 == 0 for s, d, _ in PAIRS_420)
    assert [p[2] for p in PAIRS_ODD] == [p[2] for p in PAIRS_422] == [p[2] for p in PAIRS_420] == [STAGED] * 9 + [DIRECT] * 3
    assert sorted(c[0] for c in FULL_CASES) == ["I420", "UYVY"] and all(c[1:] == ((540, 960), None, (1080, 1920)) for c in FULL_CASES)


def test_every_case_runs_on_the_path_it_was_chosen_for():
    """lvk_hip_fsr_obs_path (host only) gives every case's path, and -- the budgets being equal -- agrees with lvk_hip_fsr_easu_path everywhere."""
    from livevisionkit_amd import _native
    lib = _native.load()
    assert len(PATHS) == len(CASES) + len(FULL_CASES)
    for case, path in PATHS.items():
        _, _, rw, rh = region_of(case)
        assert lib.lvk_hip_fsr_obs_path(rw, rh, *case[3]) == path, case_id(case)
    for rw, rh, oh, ow in [(96, 48, 34, 66), (96, 49, 34, 66), (97, 48, 34, 66), (1920, 1080, 2160, 3840), (3840, 2160, 1080, 1920), (1920, 1080, 768, 1366),
                           (40, 24, 18, 30), (80, 40, 16, 64), (1, 1, 4096, 4096), (4096, 4096, 1, 1)]:
        assert lib.lvk_hip_fsr_obs_path(rw, rh, oh, ow) == lib.lvk_hip_fsr_easu_path(rw, rh, oh, ow) in (0, 1), (rw, rh, oh, ow)
    assert lib.lvk_hip_fsr_obs_path(96, 48, 34, 66) == STAGED and lib.lvk_hip_fsr_obs_path(0, 48, 34, 66) < 0 and lib.lvk_hip_fsr_obs_path(96, 48, 34, 0) < 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_constant_planes_stay_constant(fmt):
    """EASU's deringing clamp holds every output between the four nearest texels: constants in, the same constants out, through every up- and
    down-sampling of the chain."""
    src, dst = ((24, 40), (34, 62))
    frame = np.empty((*src, 3), np.uint8)
    frame[...] = (37, 201, 90)
    planes = egress(fmt, np.ascontiguousarray(frame[..., 0]) if fmt == "Y800" else frame)
    want = chain(fmt, planes, (0, 0, src[1], src[0]), dst)
    flat = egress(fmt, np.full(dst, 37, np.uint8) if fmt == "Y800" else np.broadcast_to(np.array((37, 201, 90), np.uint8), (*dst, 3)).copy())
    assert all(np.array_equal(w, f) for w, f in zip(want, flat))


def luma_of(fmt, planes):
    """The luma samples [rows, cols] of the planes of a YUV format"""
    if fmt in ("YUY2", "YVYU"):
        return planes[0][..., 0]
    if fmt in ("UYVY", "AYUV"):
        return planes[0][..., 1]
    return planes[0]


@pytest.mark.parametrize("fmt", ["I420", "UYVY", "I444"])
def test_the_chroma_in_moves_the_luma_out(fmt):
    """The direction analysis runs on 0.5 V + (0.5 Y + U): with the same luma plane and other chroma, at least half of the luma bytes out change (the
    packed specification gives 0.93 on this noise; 0.5 is a cap against a dead test).  A plane-by-plane scaler gives 0."""
    src, dst = (24, 40), (34, 62)
    a, b = noise(*src), noise(*src, seed=1).copy()
    b[..., 0] = a[..., 0]
    pa, pb = egress(fmt, a), egress(fmt, np.ascontiguousarray(b))
    assert np.array_equal(luma_of(fmt, pa), luma_of(fmt, pb))
    region = (0, 0, src[1], src[0])
    la, lb = luma_of(fmt, chain(fmt, pa, region, dst)), luma_of(fmt, chain(fmt, pb, region, dst))
    share = float((la != lb).mean())
    print(fmt, share)
    assert share >= 0.5, share


@pytest.mark.parametrize("fmt", CROP_FORMATS)
def test_the_region_is_used_pixel_by_pixel(fmt):
    """The region moved by one pixel in x, then in y: at least half of the written bytes of every plane change (the packed specification gives 0.99)."""
    src, dst = (24, 40), (20, 34)
    planes = inputs(fmt, src)
    masks = written_mask(fmt, *dst)
    base = chain(fmt, planes, (7, 5, 9, 11), dst)
    for moved in ((8, 5, 9, 11), (7, 6, 9, 11)):
        other = chain(fmt, planes, moved, dst)
        shares = [float((x[m] != y[m]).mean()) for x, y, m in zip(base, other, masks)]
        print(fmt, moved, shares)
        if fmt == "AYUV":
            assert min(shares) >= 0.5 * 0.75, shares           # a quarter of its bytes are the constant A
        else:
            assert min(shares) >= 0.5, shares


@pytest.mark.parametrize("fmt", F420)
def test_the_2x2_frame_by_hand(fmt):
    """(2, 2) -> (2, 2) on 4:2:0: the ingest replicates the one chroma sample over the frame, pp is (x, y) with no fraction, every tap outside the frame is
    the clamped texel, and the egress takes the 2 x 2 mean (sum + 2) >> 2 of the four scaled chroma values."""
    e = expected((fmt, (2, 2), None, (2, 2)))
    y = e["planes"][0]
    u0, v0 = (int(e["planes"][1][0, 0, 0]), int(e["planes"][1][0, 0, 1])) if fmt == "NV12" else (int(e["planes"][1][0, 0]), int(e["planes"][2][0, 0]))
    out = np.zeros((2, 2, 3), np.int64)
    for oy in range(2):
        for ox in range(2):
            taps = {}
            for name, (dx, dy) in nf.TAPS.items():
                cx, cy = min(max(ox + dx, 0), 1), min(max(oy + dy, 0), 1)
                r, g, b = nf.UNIT[y[cy, cx]], nf.UNIT[u0], nf.UNIT[v0]
                taps[name] = (r, g, b, nf.luma(r, g, b))
            pix = nf._easu_core(taps, f32(0), f32(0))
            out[oy, ox] = np.rint(pix * f32(255)).astype(np.int64)
    assert np.array_equal(e["want"][0], out[..., 0].astype(np.uint8))
    mean_u, mean_v = (int(out[..., 1].sum()) + 2) >> 2, (int(out[..., 2].sum()) + 2) >> 2
    got = (e["want"][1][0, 0, 0], e["want"][1][0, 0, 1]) if fmt == "NV12" else (e["want"][1][0, 0], e["want"][2][0, 0])
    assert (int(got[0]), int(got[1])) == (mean_u, mean_v) == (u0, v0)          # the deringing clamp holds a constant channel


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "I444"], ids=case_id)
def test_i444_is_the_packed_pass_on_the_three_stacked_planes(case):
    e = expected(case)
    stacked = np.ascontiguousarray(np.stack(e["planes"], -1))
    want = nf.fsr(stacked, nf.FMT_YUV, region_of(case), *case[3])
    assert all(np.array_equal(e["want"][i], want[..., i]) for i in range(3))


@pytest.mark.parametrize("fmt", ["I420", "NV12", "I422", "UYVY"])
def test_a_region_at_an_odd_origin_reads_the_other_chroma_phase(fmt):
    """The taps read the ingest's up-sampled chroma at FRAME coordinates.  A scaler that up-samples the chroma of the region as if the region started at
    an even pixel gives, for the region at the odd origin, the chroma of the region one lower: the specification does not."""
    src, dst = (24, 40), (20, 34)
    planes = inputs(fmt, src)
    masks = written_mask(fmt, *dst)
    odd = expected((fmt, src, (7, 5, 9, 11), dst))["want"]
    for even in ((6, 5, 9, 11), (6, 4, 9, 11)) if fmt in F420 else ((6, 5, 9, 11),):
        other = chain(fmt, planes, even, dst)
        assert all(float((x[m] != y[m]).mean()) >= 0.5 for x, y, m in zip(odd, other, masks)), even


@pytest.mark.parametrize("fmt", FORMATS)
def test_guard_survives_exactly_where_the_egress_writes_nothing(fmt):
    case = next(c for c in SIZE_CASES if c[0] == fmt and c[1] == (24, 40))
    masks = written_mask(fmt, *case[3])
    e = expected(case)
    for m, w in zip(masks, e["want"]):
        assert np.all(w[~m] == GUARD)
