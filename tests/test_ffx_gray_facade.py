"""lvk::CASFilter and lvk::FSRFilter on 8UC1 frames through the C++ facade (tests/cpp/ffx_gray_facade.cpp), alone and behind a DeblockingFilter in a
CompositeFilter, against the Python route (CASFilter.apply, FSRFilter.apply, DeblockingFilter.apply on two-dimensional tensors), which
tests/test_ffx_gray_gpu.py and tests/test_deblock_px_gpu.py hold to their definitions.  CPU: it compiles against the headers alone; GPU: it runs, the
type, format and timestamp are carried through and an 8UC1 frame of another format asserts (the driver checks both)."""
import os
import subprocess

import numpy as np
import pytest

from tests.deblock_px_cases import CASES, GRAY, expected
from tests.facade import build_facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ffx_gray_facade.cpp")


def test_facade_ffx_gray_compiles(tmp_path):
    build_facade(tmp_path, SRC)


@pytest.mark.gpu
def test_cas_and_fsr_alone_and_behind_deblocking_equal_the_python_route(tmp_path, ctx):
    import torch
    import livevisionkit_amd as lvk
    exe = build_facade(tmp_path, SRC)
    case = CASES[0]
    rows, cols, levels, bs, k, s, _ = case
    img, _, _ = expected(case, GRAY)
    oh, ow = 2 * rows, 2 * cols
    img.tofile(tmp_path / "in.bin")
    r = subprocess.run([exe, str(rows), str(cols), str(levels), str(bs), str(k), str(s), "2.0", "0.8", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ffx gray ok" in r.stdout, (r.stdout, r.stderr)
    assert "CASFilter %dx%d" % (cols, rows) in r.stdout and "FSRFilter %dx%d" % (ow, oh) in r.stdout and "CompositeFilter %dx%d" % (ow, oh) in r.stdout
    cas, fsr = lvk.CASFilter(ctx, 0.8), lvk.FSRFilter(ctx, multiplier=2.0)
    deblock = lvk.DeblockingFilter(ctx, detection_levels=levels, block_size=bs, filter_size=k, filter_scaling=s)
    frame = torch.from_numpy(img.copy()).cuda()
    sharpened, scaled = cas.apply(frame), fsr.apply(frame)
    deblock.apply(frame)
    chained = cas.apply(fsr.apply(frame))
    ctx.sync()
    deblock.close()
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    n = img.size
    assert got.size == n + 2 * oh * ow
    assert np.array_equal(got[:n].reshape(rows, cols), sharpened.cpu().numpy()), "CASFilter"
    assert np.array_equal(got[n:n + oh * ow].reshape(oh, ow), scaled.cpu().numpy()), "FSRFilter"
    assert np.array_equal(got[n + oh * ow:].reshape(oh, ow), chained.cpu().numpy()), "CompositeFilter"
    assert not np.array_equal(sharpened.cpu().numpy(), img) and not np.array_equal(chained.cpu().numpy(), cas.apply(scaled).cpu().numpy())
