"""lvk::DeblockingFilter on 8UC1 and 8UC4 frames through the C++ facade (tests/cpp/deblocking_px_facade.cpp), alone and ahead of a ScalingFilter in a
CompositeFilter, against the Python route (DeblockingFilter.apply, Context.upscale_gray / _c4, sharpen_gray / _c4), which tests/test_deblock_px_gpu.py
and tests/test_scaling_px_gpu.py hold to their specifications.  CPU: it compiles against the headers alone; GPU: it runs, the type, format and
timestamp are carried through and an 8UC4 frame of unknown format asserts (the driver checks both)."""
import os
import subprocess

import numpy as np
import pytest

from tests.deblock_px_cases import BGRA, CASES, GRAY, expected
from tests.facade import build_facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "deblocking_px_facade.cpp")


def test_facade_deblocking_px_compiles(tmp_path):
    build_facade(tmp_path, SRC)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 4])
def test_deblocking_filter_alone_and_in_a_composite_filter_equals_the_python_route(tmp_path, ctx, channels):
    import torch
    import livevisionkit_amd as lvk
    exe = build_facade(tmp_path, SRC)
    case = CASES[0]
    rows, cols, levels, bs, k, s, _ = case
    ow, oh = 200, 101
    fmt = GRAY if channels == 1 else BGRA
    img, _, info = expected(case, fmt)
    img.tofile(tmp_path / "in.bin")
    r = subprocess.run([exe, str(rows), str(cols), str(channels), str(levels), str(bs), str(k), str(s), str(ow), str(oh),
                        str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "deblocking ok" in r.stdout and "region %d %d %d %d" % info["region"] in r.stdout, (r.stdout, r.stderr)
    f = lvk.DeblockingFilter(ctx, detection_levels=levels, block_size=bs, filter_size=k, filter_scaling=s)
    alone = torch.from_numpy(img.copy()).cuda()
    f.apply(alone, fmt)
    up, sh = (ctx.upscale_gray, ctx.sharpen_gray) if channels == 1 else (ctx.upscale_c4, ctx.sharpen_c4)
    chained = sh(up(alone, (ow, oh)), 0.8)
    ctx.sync()
    f.close()
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    n = img.size
    assert got.size == n + oh * ow * channels
    assert np.array_equal(got[:n].reshape(img.shape), alone.cpu().numpy()), "DeblockingFilter"
    assert np.array_equal(got[n:].reshape(chained.shape), chained.cpu().numpy()), "CompositeFilter"
    assert not np.array_equal(got[:n].reshape(img.shape), img)
