"""CPU side of lvk_hip_deblock_apply_obs: the symbol's surface, and the conditions under which a pass of the GPU tests
(tests/test_deblock_obs_gpu.py) means something -- the specification of tests/deblock_obs_cases.py is, for I420 / NV12, the one
lvk_hip_deblock_apply_yuv420 is held to; the deblocking changes the planes (a byte-identical round trip would pass a copy kernel); GUARD survives in it
exactly where the egress writes nothing; and the closed form of the 4:2:2 pixel the kernels form equals the oracle's ingest on every 4:2:2 layout."""
import os
import re

import numpy as np
import pytest

from tests import deblock_420_cases as c420
from tests.deblock_obs_cases import (ALL_CASES, CASES, CASES_420, CASES_EVEN, CASES_ODD, F420, F422, FORMATS, FULL_CASES, GUARD, case_id, cases_of,
                                     changed_share, expected, inputs, live, oracle, written_mask)
from tests.scaling_obs_cases import ingest_422_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARGS = ["int video_format", "const void* const d_planes[3]", "const int steps[3]", "void* const o_planes[3]", "const int o_steps[3]",
        "int rows", "int cols", "int region_xywh[4]"]


def test_symbol_is_declared_bound_and_exported():
    """include/lvk_hip_deblock_obs.h declares exactly the entry, lvk_hip.h reaches it in its PART 2 through lvk_hip_deblock_420.h (inside both include
    guards), and livevisionkit_amd/_native.py binds exactly what it declares."""
    import ctypes
    from livevisionkit_amd import _native
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvk_hip_deblock_obs.h")).read(), flags=re.S)
    assert re.findall(r"\b(lvk_(?:hip|stab)_[a-z0-9_]+)\s*\(", code) == ["lvk_hip_deblock_apply_obs"] == _native.symbols_deblock_obs()
    decl = re.search(r"^int lvk_hip_deblock_apply_obs\(lvk_hip_deblock\* deb,(.*?)\);", code, re.S | re.M)
    assert decl and [a.strip() for a in decl.group(1).replace("\n", " ").split(",")] == ARGS
    h420 = open(os.path.join(ROOT, "include", "lvk_hip_deblock_420.h")).read()
    assert re.search(r'^#include "lvk_hip_deblock_obs.h"', h420, re.M) and h420.rstrip().endswith("#endif /* LVK_HIP_DEBLOCK_420_H */")
    text = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    assert re.search(r'^#include "lvk_hip_deblock_420.h"', experimental, re.M) and "lvk_hip_deblock_obs.h" not in stable
    assert "lvk_hip_deblock_apply_obs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fn = _native.load().lvk_hip_deblock_apply_obs
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 1 + len(ARGS)
    none3, zero3 = (ctypes.c_void_p * 3)(), (ctypes.c_int * 3)()
    assert fn(None, 1, none3, zero3, none3, zero3, 0, 0, None) != 0                    # a NULL handle is refused before anything is touched
    import livevisionkit_amd as lvk
    assert callable(lvk.DeblockingFilter.apply_obs)


def test_the_header_is_plain_c_whichever_header_comes_first(tmp_path):
    """C99 with -pedantic: alone, and before or after lvk_hip.h and lvk_hip_deblock_420.h."""
    import subprocess
    for heads in (("lvk_hip_deblock_obs.h",), ("lvk_hip.h", "lvk_hip_deblock_obs.h"), ("lvk_hip_deblock_obs.h", "lvk_hip.h"),
                  ("lvk_hip_deblock_420.h",), ("lvk_hip_deblock_obs.h", "lvk_hip_deblock_420.h"), ("lvk_hip.h",)):
        src = tmp_path / "dobs.c"
        src.write_text("".join('#include "%s"\n' % h for h in heads)
                       + 'int main(void) { (void)lvk_hip_deblock_apply_obs; (void)lvk_hip_deblock_apply_yuv420; (void)lvk_hip_deblock_apply; return 0; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_the_makefile_rule_lists_the_new_header_and_the_unit_is_a_source():
    text = open(os.path.join(ROOT, "livevisionkit_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^%\.o: %\.hip (.*)$", text, re.M).group(1).split()
    for h in ("deblock_core.hpp", "obs_planes.hpp", "obs_sinks.hpp", "../../include/lvk_hip_deblock_obs.h"):
        assert h in rule, h
    assert re.search(r"^SRCS = \$\(wildcard \*\.hip\)$", text, re.M) and os.path.exists(os.path.join(ROOT, "livevisionkit_amd", "csrc", "deblock_obs.hip"))


def test_the_case_list_is_the_one_the_tests_mean():
    assert len(FORMATS) == 16 and len(CASES) == sum(len(cases_of(f)) for f in FORMATS)
    assert len(CASES_EVEN) == 10 and len(CASES_ODD) == 4 and len(CASES_420) == len(c420.CASES) - 1 and all(c[0] < 1080 for c in CASES_420)
    assert all(c[1] % 2 == 0 for f, c in ALL_CASES if f in F422) and all((c[0] | c[1]) % 2 == 0 for f, c in ALL_CASES if f in F420)
    assert sorted(f for f, _ in FULL_CASES) == ["I444", "UYVY"] and all(c[:2] == (1080, 1920) for _, c in FULL_CASES)
    assert {c[1] for c in CASES_EVEN} >= {254, 258} and 257 in {c[1] for c in CASES_ODD}       # either side of the 256-column strip


@pytest.mark.parametrize("fmt", ["I420", "NV12", "I40A"])
@pytest.mark.parametrize("case", CASES_420, ids=c420.case_id)
def test_the_420_specification_is_the_one_of_apply_yuv420(case, fmt):
    e, e420 = expected(fmt, case), c420.expected(case)
    want = c420.as_nv12(e420["want"]) if fmt == "NV12" else e420["want"]
    assert len(want) == len(e["want"]) and all(np.array_equal(a, b) for a, b in zip(want, e["want"]))
    assert np.array_equal(e["packed"], e420["packed"]) and e["info"]["region"] == e420["info"]["region"]


@pytest.mark.parametrize("fc", [fc for fc in CASES if fc[0] not in F420], ids=case_id)
def test_the_deblocking_changes_the_planes(fc):
    """Liveness: against the plain ingest -> egress round trip.  The smallest share of written bytes that differ, found on the CPU, is 19 % (AYUV 3 x 6);
    15 % is a cap against a dead test, not a tolerance.  The 2 x 2 case -- one block, one keep level -- is the round trip."""
    fmt, case = fc
    share = changed_share(fmt, case)
    print(case_id(fc), "%.3f" % share)
    if not live(case):
        assert share == 0.0
    elif fmt == "Y800":
        assert share > 0.0
    else:
        assert share >= 0.15, share


@pytest.mark.parametrize("fmt", FORMATS)
def test_guard_survives_exactly_where_the_egress_writes_nothing(fmt):
    for case in cases_of(fmt)[3:6]:
        masks = written_mask(fmt, *case[:2])
        e = expected(fmt, case)
        for m, w, t in zip(masks, e["want"], e["trip"]):
            assert np.all(w[~m] == GUARD) and np.all(t[~m] == GUARD)
            differ = (w != GUARD) | (t != GUARD)                   # a byte both leave at GUARD would be an unwritten one
            assert np.all(differ[m]) or differ[m].mean() > 0.98, fmt


def twin_pixel(fmt, planes, x, y):
    """ObsSrc<422, .>::pixel of csrc/deblock_obs.hip, byte by byte: the pair's own sample weighs 3, the neighbouring pair's 1, the pair index clamped"""
    cols = planes[0].shape[1]
    cc, c = cols // 2, x // 2
    cf = min(c + 1, cc - 1) if x & 1 else max(c - 1, 0)
    if fmt in ("I422", "I42A"):
        lum, un, uf, vn, vf = planes[0][y, x], planes[1][y, c], planes[1][y, cf], planes[2][y, c], planes[2][y, cf]
    else:
        row = planes[0][y].reshape(-1)
        yoff, uoff, voff = {"YUY2": (0, 1, 3), "YVYU": (0, 3, 1), "UYVY": (1, 0, 2)}[fmt]
        lum, un, uf, vn, vf = row[2 * x + yoff], row[4 * c + uoff], row[4 * cf + uoff], row[4 * c + voff], row[4 * cf + voff]
    return int(lum), (int(uf) + 3 * int(un) + 2) >> 2, (int(vf) + 3 * int(vn) + 2) >> 2


@pytest.mark.parametrize("fmt", F422)
def test_the_kernels_422_pixel_is_the_oracles_ingest(fmt):
    """(other + 3 * nearer + 2) >> 2 with the edge sample replicated: the row form (tests/scaling_obs_cases.up2x_row) on every even case below 1080p,
    the kernel's own per-pixel indexing on the small ones."""
    o = oracle()
    for case in CASES_EVEN:
        planes = inputs(fmt, case)
        packed = o.ingest_obs(fmt, list(planes))
        assert np.array_equal(ingest_422_twin(fmt, planes), packed), case
        if case[0] * case[1] <= 17 * 34:
            for y in range(case[0]):
                for x in range(case[1]):
                    assert twin_pixel(fmt, planes, x, y) == tuple(int(v) for v in packed[y, x]), (case, x, y)
