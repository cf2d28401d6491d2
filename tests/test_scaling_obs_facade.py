"""lvk::ScalingFilter::apply(VideoFrameOBS, VideoFrameOBS) of the C++ facade (include/lvk/LiveVisionKit.hpp, tests/cpp/scaling_obs_facade.cpp): one format
of each family, at an upscale size and at equal sizes, against the specification of tests/scaling_obs_cases.py.  CPU: it compiles; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests.scaling_obs_cases import SIZES_420, SIZES_422, SIZES_444, case_id, expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scaling_obs_facade.cpp")

# one format of each family: an upscale with odd sizes where the format takes them, and the equal-size route across the 256-column strip
CASES = [(f, *pair, 0.8) for f, pairs in (("NV12", SIZES_420), ("UYVY", SIZES_422), ("I422", SIZES_422), ("I444", SIZES_444), ("AYUV", SIZES_444),
                                           ("BGR3", SIZES_444), ("BGRA", SIZES_444), ("Y800", SIZES_444))
         for pair in ((pairs[2], pairs[4]) if f == "NV12" else (pairs[5], pairs[-6]))]


def test_facade_scaling_obs_compiles(tmp_path):
    from tests.facade import build_facade
    build_facade(tmp_path, SRC)


def tight(planes):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_facade_apply_obs(ctx, tmp_path, case):
    from tests.facade import build_facade
    exe = build_facade(tmp_path, SRC)
    fmt, (rows, cols), (orows, ocols), sharpness = case
    e = expected(case, "smooth")
    tight(e["planes"]).tofile(tmp_path / "in.bin")
    r = subprocess.run([exe, str(ctx.VIDEO_FORMATS[fmt]), str(rows), str(cols), str(orows), str(ocols), str(sharpness), str(tmp_path / "in.bin"),
                        str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scale obs ok: %d %dx%d -> %dx%d" % (ctx.VIDEO_FORMATS[fmt], cols, rows, ocols, orows) in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    assert np.array_equal(got, tight(e["want"]))               # GUARD where the egress writes nothing: the program fills its output with it first
