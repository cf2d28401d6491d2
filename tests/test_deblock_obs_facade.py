"""lvk::DeblockingFilter::apply(VideoFrameOBS, VideoFrameOBS) of the C++ facade (include/lvk/DeblockingFilter.hpp, tests/cpp/deblocking_obs_facade.cpp):
one format of each family against the specification of tests/deblock_obs_cases.py.  CPU: it compiles; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests.deblock_obs_cases import CASES_420, CASES_EVEN, CASES_ODD, case_id, expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "deblocking_obs_facade.cpp")

# one format of each family: area tables with rows and columns outside the region, and an odd size where the format takes one
CASES = [("NV12", CASES_420[6]), ("UYVY", CASES_EVEN[5]), ("I422", CASES_EVEN[9]), ("I444", CASES_ODD[3]), ("AYUV", CASES_ODD[2]), ("BGR3", CASES_ODD[3]),
         ("BGRA", CASES_EVEN[5]), ("Y800", CASES_ODD[2])]


def test_facade_deblocking_obs_compiles(tmp_path):
    from tests.facade import build_facade
    build_facade(tmp_path, SRC)


def tight(planes):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])


@pytest.mark.gpu
@pytest.mark.parametrize("fc", CASES, ids=case_id)
def test_facade_apply_obs(ctx, tmp_path, fc):
    from tests.facade import build_facade
    exe = build_facade(tmp_path, SRC)
    fmt, case = fc
    rows, cols, levels, bs, k, s = case
    e = expected(fmt, case)
    tight(e["planes"]).tofile(tmp_path / "in.bin")
    r = subprocess.run([exe, str(ctx.VIDEO_FORMATS[fmt]), str(rows), str(cols), str(levels), str(bs), str(k), repr(s), str(tmp_path / "in.bin"),
                        str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    region = e["info"]["region"]
    assert r.returncode == 0 and "deblock obs ok: %d %dx%d region %dx%d" % (ctx.VIDEO_FORMATS[fmt], cols, rows, region[2], region[3]) in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    assert np.array_equal(got, tight(e["want"]))               # GUARD where the egress writes nothing: the program fills its output with it first
