"""lvk::CASFilter::apply(VideoFrame420, VideoFrame420) and apply(VideoFrameOBS, VideoFrameOBS) of the C++ facade (include/lvk/CASFilter.hpp,
tests/cpp/cas_obs_facade.cpp): both 4:2:0 layouts and one format of each other family against the specification of tests/cas_obs_cases.py.
CPU: it compiles; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests.cas_obs_cases import case_id, expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cas_obs_facade.cpp")
SHARPNESS = 0.8

# (entry, format, size): the 4:2:0 planes through VideoFrame420, the others through VideoFrameOBS; an odd size where the format takes one
CASES = [("420", "I420", (68, 258)), ("420", "NV12", (18, 34)), ("obs", "UYVY", (67, 258)), ("obs", "I444", (67, 257)), ("obs", "AYUV", (17, 35)),
         ("obs", "BGRA", (17, 34)), ("obs", "Y800", (67, 257))]


def test_facade_cas_obs_compiles(tmp_path):
    from tests.facade import build_facade
    build_facade(tmp_path, SRC)


def tight(planes):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % (c[0], case_id(c[1:])))
def test_facade_apply(ctx, tmp_path, case):
    from tests.facade import build_facade
    exe = build_facade(tmp_path, SRC)
    entry, fmt, size = case
    rows, cols = size
    e = expected(fmt, size, SHARPNESS)
    tight(e["planes"]).tofile(tmp_path / "in.bin")
    layout = (1 if fmt == "NV12" else 0) if entry == "420" else ctx.VIDEO_FORMATS[fmt]
    r = subprocess.run([exe, entry, str(layout), str(rows), str(cols), repr(SHARPNESS), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cas %s ok: %d %dx%d" % (entry, layout, cols, rows) in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    assert np.array_equal(got, tight(e["want"]))               # GUARD where the egress writes nothing: the program fills its output with it first
