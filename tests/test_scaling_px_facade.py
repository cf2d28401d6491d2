"""lvk::ScalingFilter on 8UC1 and 8UC4 frames through the C++ facade (tests/cpp/scaling_px_facade.cpp), alone and inside a CompositeFilter, against the
Python route (Context.upscale_gray / _c4, sharpen_gray / _c4), which tests/test_scaling_px_gpu.py holds to the definitions.  CPU: it compiles against the
headers alone; GPU: it runs, and the type, format and timestamp are carried through (the driver checks them)."""
import os
import subprocess

import numpy as np
import pytest

from tests import scaling_px_cases as cases
from tests.facade import build_facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scaling_px_facade.cpp")


def test_facade_scaling_px_compiles(tmp_path):
    build_facade(tmp_path, SRC)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 4])
def test_scaling_filter_alone_and_in_a_composite_filter_equals_the_python_route(tmp_path, ctx, channels):
    import torch
    exe = build_facade(tmp_path, SRC)
    rows, cols, ow, oh, sharpness = 67, 131, 200, 101, 0.8
    f = cases.frame(rows, cols)
    f = np.ascontiguousarray(f[..., 0]) if channels == 1 else f
    f.tofile(tmp_path / "in.bin")
    r = subprocess.run([exe, str(rows), str(cols), str(ow), str(oh), str(channels), str(sharpness), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "scaling ok" in r.stdout, (r.stdout, r.stderr)
    up, sh = (ctx.upscale_gray, ctx.sharpen_gray) if channels == 1 else (ctx.upscale_c4, ctx.sharpen_c4)
    alone = sh(up(torch.from_numpy(f).cuda(), (ow, oh)), sharpness)
    chained = sh(up(alone, (ow, oh)), 0.3)
    ctx.sync()
    got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape((2, oh, ow) + f.shape[2:])
    assert np.array_equal(got[0], alone.cpu().numpy()), "ScalingFilter"
    assert np.array_equal(got[1], chained.cpu().numpy()), "CompositeFilter"
    assert not np.array_equal(got[0], got[1])
