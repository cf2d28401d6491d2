"""lvk::HostFrameOBS and StabilizationFilter::apply(const HostFrameOBS&, HostFrameOBS&) of the C++ facade (include/lvk/LiveVisionKit.hpp) driven by
tests/cpp/obs_host_facade.cpp: UYVY and BGRA host frames through the facade against the C-ABI stream (lvk_hip_stab_push_obs on the same frames).
CPU: the driver compiles against the headers and links; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests.facade import build_facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "obs_host_facade.cpp")


def test_facade_obs_host_compiles(tmp_path):
    build_facade(tmp_path, SRC)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["UYVY", "BGRA"])
def test_facade_obs_host_stream_equals_the_c_abi_stream(tmp_path, ctx, oracle, name):
    import torch
    import livevisionkit_amd as lvk
    from tests import synth
    from tests.test_push_obs_edges_gpu import _source
    exe = build_facade(tmp_path, SRC)
    rows, cols, n, delay = 540, 960, 12, 3
    clip, _ = synth.make_clip(rows, cols, n, seed=53, jitter=1.0)
    # the settings the driver configures (the plugin's homography preset, relaxed quality assurance: real homographies are applied)
    s = lvk.StabilizationFilterSettings.obs_preset("homography", strict=False, predictive_samples=delay, min_scene_quality=0.3, min_tracking_quality=0.2)
    gst = lvk.StabilizationFilter(lvk.StabilizationFilterSettings(), context=ctx); gst.configure(s); gst.set_overlap(True)
    want = []
    with open(tmp_path / "clip.bin", "wb") as f:
        for i, fr in enumerate(clip):
            planes = oracle.egress_obs(name, _source(name, fr))
            for p in planes:
                f.write(p.tobytes())
            out = [torch.zeros(p.shape, dtype=torch.uint8, device="cuda") for p in planes]
            got, ts = gst.apply_obs(name, [torch.from_numpy(p).cuda() for p in planes], timestamp=500 + i, out=out)
            ctx.sync()
            if got is not None:
                assert ts == 500 + i - delay
                want.append(np.concatenate([p.cpu().numpy().reshape(-1) for p in got]))
    assert len(want) == n - delay
    st = gst.stats()
    assert st.trust > 0.1 and st.n_matched >= 50, f"trust {st.trust:.2f}: the compared frames carry no stabilizing warp"
    gst.close()
    r = subprocess.run([exe, str(lvk.Context.VIDEO_FORMATS[name]), str(rows), str(cols), str(n), str(delay), str(tmp_path / "clip.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and f"stream ok: {len(want)} frames" in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    assert got.size == sum(w.size for w in want)
    off = 0
    for k, w in enumerate(want):
        assert np.array_equal(got[off:off + w.size], w), (name, k)
        off += w.size
