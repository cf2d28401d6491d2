"""lvk::VideoFrameOBS and LCFilter::apply(VideoFrameOBS, VideoFrameOBS) of the C++ facade (include/lvk/LiveVisionKit.hpp, include/lvk/LCFilter.hpp,
tests/cpp/lens_obs_facade.cpp): upload -> apply -> download against the Python route (LCFilter.apply_obs) and the specification of
tests/lens_obs_cases.py.  CPU: it compiles; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests.lens_obs_cases import filter_expected, params_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lens_obs_facade.cpp")
SIZE, PROFILE, KIND = (66, 258), 0, "smooth"


def test_facade_lens_obs_compiles(tmp_path):
    from tests.facade import build_facade
    build_facade(tmp_path, SRC)


def tight(planes):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["UYVY", "I444", "BGR3", "NV12"])
def test_facade_apply_obs_equals_the_python_route(tmp_path, ctx, fmt):
    import torch
    import livevisionkit_amd as lvk
    from tests.facade import build_facade
    exe = build_facade(tmp_path, SRC)
    e = filter_expected(fmt, SIZE, PROFILE, True, KIND)
    params = params_of(PROFILE, *SIZE)
    tight(e["planes"]).tofile(tmp_path / "in.bin")
    r = subprocess.run([exe, str(ctx.VIDEO_FORMATS[fmt]), "1", ",".join(repr(v) for v in params), str(SIZE[0]), str(SIZE[1]),
                        str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lens obs ok: %d %dx%d" % (ctx.VIDEO_FORMATS[fmt], SIZE[1], SIZE[0]) in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    f = lvk.LCFilter(params, True, context=ctx)
    try:
        out = f.apply_obs(fmt, [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in e["planes"]])
        ctx.sync()
        python = tight([o.cpu().numpy() for o in out])
    finally:
        f.close()
    assert np.array_equal(got, python)
    assert np.array_equal(got, tight(e["want"]))
