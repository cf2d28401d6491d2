"""lvk::ScalingFilter::apply(VideoFrame420, VideoFrame420) of the C++ facade (include/lvk/LiveVisionKit.hpp, tests/cpp/scaling_420_facade.cpp): I420 and
NV12 planes in and out, at an upscale size and at equal sizes, against the Python route (Context.scale_yuv420) and the specification of
tests/scaling_420_cases.py.  CPU: it compiles; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests.scaling_420_cases import C_258, C_P254, as_nv12, case_id, expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scaling_420_facade.cpp")


def test_facade_scaling_420_compiles(tmp_path):
    from tests.facade import build_facade
    build_facade(tmp_path, SRC)


def tight(planes):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])


@pytest.mark.gpu
@pytest.mark.parametrize("nv12", [0, 1], ids=["i420", "nv12"])
@pytest.mark.parametrize("case", [C_258, C_P254], ids=case_id)
def test_facade_apply_420(ctx, tmp_path, case, nv12):
    import torch
    from tests.facade import build_facade
    exe = build_facade(tmp_path, SRC)
    e = expected(case, "smooth")
    rows, cols, orows, ocols, sharpness = case
    planes = as_nv12(e["planes"]) if nv12 else e["planes"]
    tight(planes).tofile(tmp_path / "planes.bin")
    r = subprocess.run([exe, str(nv12), str(rows), str(cols), str(orows), str(ocols), str(sharpness), str(tmp_path / "planes.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scale 420 ok: %dx%d -> %dx%d" % (cols, rows, ocols, orows) in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    python_route = ctx.scale_yuv420(*[torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes], size=(ocols, orows), sharpness=sharpness)
    ctx.sync()
    assert np.array_equal(got, tight([p.cpu().numpy() for p in python_route]))
    assert np.array_equal(got, tight(as_nv12(e["want"]) if nv12 else e["want"]))
