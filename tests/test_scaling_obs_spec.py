"""CPU side of lvk_hip_scale_obs: the symbol's surface, and the conditions under which a pass of the GPU tests
(tests/test_scaling_obs_gpu.py) means something -- the specification of tests/scaling_obs_cases.py is, for I420 / NV12, the one lvk_hip_scale_yuv420 is
held to; its all-border case is the ingest -> egress round trip; GUARD survives in it exactly where the egress writes nothing; the sharpening changes the
planes; and the closed form of the 4:2:2 chroma up-sampling the planar kernel source uses equals the oracle's ingest on every 4:2:2 layout."""
import os
import re

import numpy as np
import pytest

from tests import scaling_420_cases as c420
from tests.scaling_obs_cases import (ALL_CASES, CASES, ENDS, F420, F422, FORMATS, GUARD, SIZES_420, SIZES_422, case_id, chain, equal_sizes, expected,
                                     ingest_422_twin, inputs, oracle, sizes_of, textures_of, written_mask)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARGS = ["int video_format", "const void* const d_planes[3]", "const int steps[3]", "int src_rows", "int src_cols",
        "void* const o_planes[3]", "const int o_steps[3]", "int dst_rows", "int dst_cols", "float sharpness"]


def test_symbol_is_declared_bound_and_exported():
    """include/lvk_hip_scaling_obs.h declares exactly the entry, lvk_hip.h reaches it in its PART 2 through lvk_hip_scaling_420.h (inside both include
    guards), and livevisionkit_amd/_native.py binds exactly what it declares."""
    import ctypes
    from livevisionkit_amd import _native
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvk_hip_scaling_obs.h")).read(), flags=re.S)
    assert re.findall(r"\b(lvk_(?:hip|stab)_[a-z0-9_]+)\s*\(", code) == ["lvk_hip_scale_obs"] == _native.symbols_scaling_obs()
    decl = re.search(r"^int lvk_hip_scale_obs\(lvk_hip_ctx\* ctx,(.*?)\);", code, re.S | re.M)
    assert decl and [a.strip() for a in decl.group(1).replace("\n", " ").split(",")] == ARGS
    h420 = open(os.path.join(ROOT, "include", "lvk_hip_scaling_420.h")).read()
    assert re.search(r'^#include "lvk_hip_scaling_obs.h"', h420, re.M) and h420.rstrip().endswith("#endif /* LVK_HIP_SCALING_420_H */")
    text = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    assert re.search(r'^#include "lvk_hip_scaling_420.h"', experimental, re.M) and "lvk_hip_scaling_obs.h" not in stable
    assert "lvk_hip_scale_obs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fn = _native.load().lvk_hip_scale_obs
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 1 + len(ARGS)
    none3, zero3 = (ctypes.c_void_p * 3)(), (ctypes.c_int * 3)()
    assert fn(None, 1, none3, zero3, 0, 0, none3, zero3, 0, 0, 0.5) != 0               # a NULL context is refused before anything is touched
    import livevisionkit_amd as lvk
    assert callable(lvk.Context.scale_obs)


def test_the_header_is_plain_c_whichever_header_comes_first(tmp_path):
    """C99 with -pedantic: alone, and before or after lvk_hip.h and lvk_hip_scaling_420.h."""
    import subprocess
    for heads in (("lvk_hip_scaling_obs.h",), ("lvk_hip.h", "lvk_hip_scaling_obs.h"), ("lvk_hip_scaling_obs.h", "lvk_hip.h"),
                  ("lvk_hip_scaling_420.h",), ("lvk_hip_scaling_obs.h", "lvk_hip_scaling_420.h"), ("lvk_hip.h",)):
        src = tmp_path / "sobs.c"
        src.write_text("".join('#include "%s"\n' % h for h in heads)
                       + 'int main(void) { (void)lvk_hip_scale_obs; (void)lvk_hip_scale_yuv420; (void)lvk_hip_sharpen; return 0; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_the_makefile_rule_lists_the_new_headers_and_the_unit_is_a_source():
    text = open(os.path.join(ROOT, "livevisionkit_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^%\.o: %\.hip (.*)$", text, re.M).group(1).split()
    for h in ("rcas_src.hpp", "obs_planes.hpp", "obs_sinks.hpp", "../../include/lvk_hip_scaling_obs.h"):
        assert h in rule, h
    assert re.search(r"^SRCS = \$\(wildcard \*\.hip\)$", text, re.M) and os.path.exists(os.path.join(ROOT, "livevisionkit_amd", "csrc", "scaling_obs.hip"))


def test_the_case_list_is_the_one_the_tests_mean():
    assert len(FORMATS) == 16 and len(CASES) == sum(len(sizes_of(f)) for f in FORMATS)
    assert len(SIZES_420) == 5 and all(c[1][1] % 2 == 0 and c[2][1] % 2 == 0 for c in ALL_CASES if c[0] in F422)
    assert sorted({c[0] for c in ENDS}) == ["BGR3", "I444", "UYVY"] and len(ENDS) == 12 and {c[3] for c in ENDS} == {0.0, 1.0}
    assert {equal_sizes(c) for c in ENDS} == {True, False}
    for cols4 in range(4):                                         # every cols % 4 and every rows % 4 among the equal-size cases
        assert [c for c in CASES if c[0] == "I444" and equal_sizes(c) and c[1][1] % 4 == cols4]
        assert [c for c in CASES if c[0] == "I444" and equal_sizes(c) and c[1][0] % 4 == cols4]


@pytest.mark.parametrize("kind", c420.TEXTURES)
@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("I420", "NV12")], ids=case_id)
def test_the_420_specification_is_the_one_of_scale_yuv420(case, kind):
    fmt, src, dst, sharpness = case
    e = expected(case, kind)
    want, packed, scaled = c420.chain(c420.texture(kind, *src, c420.SEED), *dst, sharpness)
    want = c420.as_nv12(want) if fmt == "NV12" else want
    assert len(want) == len(e["want"]) and all(np.array_equal(a, b) for a, b in zip(want, e["want"]))
    assert np.array_equal(packed, e["packed"]) and np.array_equal(scaled, e["scaled"])


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_all_border_case_is_the_ingest_egress_round_trip(fmt):
    case = (fmt, (2, 2), (2, 2), 0.8)
    assert case in CASES
    for kind in textures_of(case):
        e = expected(case, kind)
        round_trip, _, _ = chain(fmt, e["planes"], (2, 2), 0.8, sharpen=False)
        assert all(np.array_equal(a, b) for a, b in zip(round_trip, e["want"])), kind


@pytest.mark.parametrize("fmt", FORMATS)
def test_guard_survives_exactly_where_the_egress_writes_nothing(fmt):
    """... and the cases are live: the sharpening changes the planes, an upscale is no copy of the input."""
    mine = [c for c in CASES if c[0] == fmt]
    for case in ([c for c in mine if not equal_sizes(c)][-2], [c for c in mine if equal_sizes(c) and c[1][0] >= 14][0]):
        dst = case[2]
        masks = written_mask(fmt, *dst)
        a, b = expected(case, "random")["want"], expected(case, "smooth")["want"]
        for m, pa, pb in zip(masks, a, b):
            assert np.all(pa[~m] == GUARD) and np.all(pb[~m] == GUARD)
            differ = (pa != GUARD) | (pb != GUARD)                 # a byte both textures leave at GUARD would be an unwritten one
            assert np.all(differ[m]) or (differ[m].mean() > 0.99), fmt
        unsharpened, _, _ = chain(fmt, expected(case, "smooth")["planes"], dst, case[3], sharpen=False)
        assert any(not np.array_equal(u, w) for u, w in zip(unsharpened, b)), case_id(case)


@pytest.mark.parametrize("fmt", F422)
def test_up2x_closed_form_is_the_oracles_422_ingest(fmt):
    """(other + 3 * nearer + 2) >> 2 with the edge sample replicated, per row: what PlaneSrc<422, .> of csrc/scaling_obs.hip forms in registers."""
    o = oracle()
    for size in sorted({s for s, _ in SIZES_422 if s[1] <= 34} | {(5, 10), (8, 10)}):
        for kind in ("random", "smooth"):
            planes = inputs(fmt, size, kind)
            assert np.array_equal(ingest_422_twin(fmt, planes), o.ingest_obs(fmt, list(planes))), (size, kind)
