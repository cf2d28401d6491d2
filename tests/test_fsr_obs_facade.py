"""lvk::FSRFilter::apply(VideoFrame420, VideoFrame420) and apply(VideoFrameOBS, VideoFrameOBS) of the C++ facade (include/lvk/FSRFilter.hpp,
tests/cpp/fsr_obs_facade.cpp): both overloads in each settings mode -- the multiplier alone, and an explicit output size with crops --, the skip path,
the assertions and the chain FSRFilter -> CASFilter on VideoFrameOBS, against the planes of tests/fsr_obs_cases.py.  CPU: it compiles; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests.cas_obs_cases import chain as cas_chain
from tests.fsr_obs_cases import case_id, expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fsr_obs_facade.cpp")
SHARPNESS = 0.8

BY_MULTIPLIER = ((24, 40), None, (18, 30), 0.75)             # 0.75 x: a staged downscale
BY_SIZE = ((24, 40), (7, 5, 9, 11), (20, 34), 0.0)           # an explicit size, crops 7, 5, 24, 8
DIRECT = ((66, 130), (3, 1, 120, 60), (16, 32), 0.0)         # the direct route
# (entry, format, (source, region, output, multiplier), sharpen)
CASES = [("420", "I420", BY_MULTIPLIER, False), ("420", "NV12", BY_SIZE, False), ("420", "I420", DIRECT, False),
         ("obs", "UYVY", BY_MULTIPLIER, False), ("obs", "I444", BY_SIZE, False), ("obs", "AYUV", DIRECT, False), ("obs", "BGRA", BY_SIZE, False),
         ("obs", "Y800", BY_SIZE, False), ("obs", "I420", BY_SIZE, False), ("obs", "UYVY", BY_SIZE, True), ("obs", "I444", DIRECT, True)]


def test_facade_fsr_obs_compiles(tmp_path):
    from tests.facade import build_facade
    build_facade(tmp_path, SRC)


def tight(planes):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s%s" % (c[0], case_id((c[1],) + c[2][:3]), "-cas" if c[3] else ""))
def test_facade_apply(ctx, tmp_path, case):
    from tests.facade import build_facade
    exe = build_facade(tmp_path, SRC)
    entry, fmt, (src, region, dst, multiplier), sharpen = case
    rows, cols = src
    e = expected((fmt, src, region, dst))
    want = cas_chain(fmt, e["want"], SHARPNESS) if sharpen else e["want"]
    tight(e["planes"]).tofile(tmp_path / "in.bin")
    layout = (1 if fmt == "NV12" else 0) if entry == "420" else ctx.VIDEO_FORMATS[fmt]
    rx, ry, rw, rh = region or (0, 0, cols, rows)
    crop = [rx, ry, cols - rx - rw, rows - ry - rh]
    args = [entry, layout, rows, cols, dst[0], dst[1], repr(multiplier), *crop, repr(SHARPNESS if sharpen else -1.0)]
    r = subprocess.run([exe, *[str(a) for a in args], str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fsr %s ok: %d %dx%d -> %dx%d" % (entry, layout, cols, rows, dst[1], dst[0]) in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    assert np.array_equal(got, tight(want))                    # GUARD where the egress writes nothing: the program fills its output with it first
