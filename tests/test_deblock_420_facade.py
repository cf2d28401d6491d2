"""lvk::DeblockingFilter::apply(VideoFrame420, VideoFrame420) of the C++ facade (include/lvk/DeblockingFilter.hpp, tests/cpp/deblocking_420_facade.cpp):
I420 and NV12 planes in and out against the specification of tests/deblock_420_cases.py.  CPU: it compiles; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests.deblock_420_cases import as_nv12, oracle, specification
from tests.deblock_px_cases import blocky

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "deblocking_420_facade.cpp")


def test_facade_deblocking_420_compiles(tmp_path):
    from tests.facade import build_facade
    build_facade(tmp_path, SRC)


def tight(planes):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])


@pytest.mark.gpu
@pytest.mark.parametrize("nv12", [0, 1], ids=["i420", "nv12"])
@pytest.mark.parametrize("rows,cols,levels,bs,k,s", [(66, 130, 3, 16, 5, 3.0), (360, 640, 3, 16, 5, 4.0)])
def test_facade_apply_420(tmp_path, rows, cols, levels, bs, k, s, nv12):
    from tests.facade import build_facade
    exe = build_facade(tmp_path, SRC)
    planes = oracle().egress_yuv420(blocky(rows, cols, seed=rows * 7 + cols + 3, block=bs))
    want, info, _ = specification(planes, levels, bs, k, s)
    tight(as_nv12(planes) if nv12 else planes).tofile(tmp_path / "planes.bin")
    r = subprocess.run([exe, str(nv12), str(rows), str(cols), str(levels), str(bs), str(k), str(s), str(tmp_path / "planes.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "apply 420 ok: region %d %d %d %d" % info["region"] in r.stdout, (r.stdout, r.stderr)
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.uint8), tight(as_nv12(want) if nv12 else want))
