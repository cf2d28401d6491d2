"""One-channel (GRAY / Y800) frames through the C++ facade (tests/cpp/gray_facade.cpp): FrameIngest::SelectY800 -> upload_obs_frame ->
StabilizationFilter::apply -> download_ocl_frame, and WarpMesh::apply / the two lvk::remap launchers on an 8UC1 frame, against the Python route
(livevisionkit_amd.StabilizationFilter.apply on [rows, cols] tensors, Context.*_gray), which tests/test_gray_stabilizer_gpu.py and
tests/test_gray_remap_gpu.py hold to the oracle.  CPU: it compiles against the headers alone; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests.facade import build_facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "gray_facade.cpp")


def test_facade_gray_compiles(tmp_path):
    build_facade(tmp_path, SRC)


@pytest.mark.gpu
def test_facade_y800_ingest_apply_egress_equals_the_python_route(tmp_path, ctx):
    import torch
    import livevisionkit_amd as lvk
    from tests import clipgen
    exe = build_facade(tmp_path, SRC)
    rows, cols, n, delay = 270, 480, 12, 3
    clip = clipgen.Clip(rows, cols, n, device="cuda")
    planes = [clip.render444(i)[..., 0].contiguous() for i in range(n)]
    with open(tmp_path / "clip.bin", "wb") as f:
        for p in planes:
            f.write(p.cpu().numpy().tobytes())
    r = subprocess.run([exe, str(rows), str(cols), str(n), str(delay), str(tmp_path / "clip.bin"), str(tmp_path / "out.bin"), str(tmp_path / "ops.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and f"stream ok: {n - delay} frames" in r.stdout, (r.stdout, r.stderr)

    # the Python route, the same preset (tests/cpp/gray_facade.cpp)
    s = lvk.StabilizationFilterSettings.obs_preset("homography", strict=False, predictive_samples=delay, min_scene_quality=0.3, min_tracking_quality=0.2)
    gst = lvk.StabilizationFilter(s, context=ctx)
    want = []
    for i, p in enumerate(planes):
        out, ts = gst.apply(p, timestamp=500 + i); ctx.sync()
        if out is not None:
            assert ts == 500 + i - delay
            want.append(out.cpu().numpy())
    assert gst.stats().trust > 0.1, "the compared frames must carry a live warp"
    gst.close()
    got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(-1, rows, cols)
    assert len(got) == len(want) == n - delay
    for k, w in enumerate(want):
        assert np.array_equal(got[k], w), k

    ops = np.fromfile(tmp_path / "ops.bin", np.uint8).reshape(3, rows, cols)
    mesh = np.array([0.01 * ((i * 7) % 5 - 2) for i in range(18)], np.float32).reshape(3, 3, 2)
    H = np.array([0.98, 0.05, 3.25, -0.04, 1.01, -2.5, 1e-5, 0.0, 1.0], np.float32)
    offs = torch.empty((rows, cols, 2), dtype=torch.float32, device="cuda"); offs[..., 0] = 1.37; offs[..., 1] = -0.61
    py = [ctx.warpmesh_apply_gray(planes[0], mesh, bg=77), ctx.remap_homography_gray(planes[0], H, bg=77), ctx.remap_map_gray(planes[0], offs, bg=77)]
    ctx.sync()
    for name, a, b in zip(("WarpMesh::apply", "remap(homography)", "remap(offset map)"), ops, py):
        assert np.array_equal(a, b.cpu().numpy()), name
