"""Four-channel (BGRA / RGBA / BGRX) frames through the C++ facade (tests/cpp/c4_facade.cpp): FrameIngest::SelectRGBX -> upload_obs_frame ->
StabilizationFilter::apply -> download_ocl_frame, and WarpMesh::apply / the two lvk::remap launchers on an 8UC4 frame, against the Python route
(livevisionkit_amd.StabilizationFilter.apply on [rows, cols, 4] tensors, Context.*_c4), which tests/test_c4_stabilizer_gpu.py and
tests/test_c4_remap_gpu.py hold to the oracle.  CPU: it compiles against the headers alone; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests.facade import build_facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "c4_facade.cpp")
BG = (77, 201, 5, 130)


def test_facade_c4_compiles(tmp_path):
    build_facade(tmp_path, SRC)


@pytest.mark.gpu
@pytest.mark.parametrize("video_format", ["BGRA", "RGBA", "BGRX"])
def test_facade_rgbx_ingest_apply_egress_equals_the_python_route(tmp_path, ctx, video_format):
    import torch
    import livevisionkit_amd as lvk
    from livevisionkit_amd import stabilization as st
    from tests import clipgen
    exe = build_facade(tmp_path, SRC)
    vf = {"RGBA": 6, "BGRA": 7, "BGRX": 8}[video_format]          # LVK_VIDEO_FORMAT_* (include/lvk_hip.h)
    header = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    assert f"#define LVK_VIDEO_FORMAT_{video_format} {vf}" in " ".join(header.split())
    fmt = st.FORMAT_RGBA if video_format == "RGBA" else st.FORMAT_BGRA
    rows, cols, n, delay = 270, 480, 12, 3
    clip = clipgen.Clip(rows, cols, n, device="cuda")
    yy, xx = torch.meshgrid(torch.arange(rows, device="cuda"), torch.arange(cols, device="cuda"), indexing="ij")
    frames = []
    for i in range(n):
        alpha = ((xx * 3 + yy * 5 + 17 * i) % 251).to(torch.uint8)            # a moving pattern that is no colour plane
        frames.append(torch.cat([clip.render444(i), alpha[..., None]], -1).contiguous())
    with open(tmp_path / "clip.bin", "wb") as f:
        for p in frames:
            f.write(p.cpu().numpy().tobytes())
    r = subprocess.run([exe, str(rows), str(cols), str(n), str(delay), str(vf), str(tmp_path / "clip.bin"), str(tmp_path / "out.bin"), str(tmp_path / "ops.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and f"stream ok: {n - delay} frames" in r.stdout, (r.stdout, r.stderr)

    # the Python route, the same preset (tests/cpp/c4_facade.cpp)
    s = lvk.StabilizationFilterSettings.obs_preset("homography", strict=False, predictive_samples=delay, min_scene_quality=0.3, min_tracking_quality=0.2)
    gst = lvk.StabilizationFilter(s, context=ctx)
    gst.set_background_alpha(66)
    want = []
    for i, p in enumerate(frames):
        out, ts = gst.apply(p, timestamp=500 + i, fmt=fmt); ctx.sync()
        if out is not None:
            assert ts == 500 + i - delay and out.shape == (rows, cols, 4) and gst.last_format == fmt
            want.append(out.cpu().numpy())
    assert gst.stats().trust > 0.1, "the compared frames must carry a live warp"
    gst.close()
    got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(-1, rows, cols, 4)
    assert len(got) == len(want) == n - delay
    for k, w in enumerate(want):
        assert np.array_equal(got[k], w), k

    ops = np.fromfile(tmp_path / "ops.bin", np.uint8).reshape(3, rows, cols, 4)
    mesh = np.array([0.01 * ((i * 7) % 5 - 2) for i in range(18)], np.float32).reshape(3, 3, 2)
    H = np.array([0.98, 0.05, 3.25, -0.04, 1.01, -2.5, 1e-5, 0.0, 1.0], np.float32)
    offs = torch.empty((rows, cols, 2), dtype=torch.float32, device="cuda"); offs[..., 0] = 1.37; offs[..., 1] = -0.61
    py = [ctx.warpmesh_apply_c4(frames[0], mesh, bg=BG), ctx.remap_homography_c4(frames[0], H, bg=BG), ctx.remap_map_c4(frames[0], offs, bg=BG)]
    ctx.sync()
    for name, a, b in zip(("WarpMesh::apply", "remap(homography)", "remap(offset map)"), ops, py):
        assert np.array_equal(a, b.cpu().numpy()), name
