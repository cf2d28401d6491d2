"""lvk::DeblockingFilter of the C++ facade (include/lvk/DeblockingFilter.hpp): the ADB filter's calls against tests/np_deblock.py, the editor's
CompositeFilter{StabilizationFilter, DeblockingFilter} against the oracle's stabilizer followed by np_deblock, and the OBS path (I420 through
upload_obs_frame -> apply -> download_ocl_frame) against the oracle's ingest / egress around np_deblock.  CPU: it compiles; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests import np_deblock as nd
from tests.facade import build_facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "deblocking_facade.cpp")


def test_facade_deblocking_filter_compiles(tmp_path):
    build_facade(tmp_path, SRC)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,fmt,levels,bs,k,s", [(270, 480, 4, 3, 16, 5, 4.0), (131, 67, 0, 5, 8, 7, 3.0), (1080, 1920, 2, 1, 16, 3, 2.0)])
def test_facade_apply_and_draw_influence(tmp_path, rows, cols, fmt, levels, bs, k, s):
    from tests.test_deblock_gpu import blocky
    exe = build_facade(tmp_path, SRC)
    img = blocky(rows, cols, seed=rows * 7 + k)
    img.tofile(tmp_path / "frame.bin")
    prefix = str(tmp_path / "out")
    r = subprocess.run([exe, "apply", str(fmt), str(rows), str(cols), str(levels), str(bs), str(k), str(s), str(tmp_path / "frame.bin"), prefix],
                       capture_output=True, text=True, timeout=120)
    want, info = nd.deblock(img, fmt, levels, bs, k, s)
    assert r.returncode == 0 and "apply ok: region %d %d %d %d" % info["region"] in r.stdout, (r.stdout, r.stderr)
    assert np.array_equal(np.fromfile(prefix + ".apply", np.uint8).reshape(rows, cols, 3), want)
    assert np.array_equal(np.fromfile(prefix + ".influence", np.uint8).reshape(rows, cols, 3), nd.draw_influence(want, fmt, info))


@pytest.mark.gpu
@pytest.mark.parametrize("with_stab", [0, 1])
def test_facade_obs_path_and_composite_chain(tmp_path, oracle, with_stab):
    from tests import oracle_lib, synth
    exe = build_facade(tmp_path, SRC)
    rows, cols, n, delay = 270, 480, 10, 3
    clip, _ = synth.make_clip(rows, cols, n, seed=61, jitter=1.0)
    ost = None
    if with_stab:
        ost = oracle_lib.OracleStabilizer(oracle, oracle_lib.preset("homography", predictive_samples=delay, min_scene_quality=0.3, min_tracking_quality=0.2))
    want = []
    with open(tmp_path / "clip.bin", "wb") as f:
        for i, fr in enumerate(clip):
            planes = oracle.egress_obs("I420", fr)
            for p in planes:
                f.write(p.tobytes())
            packed = oracle.ingest_obs("I420", planes)
            if ost is not None:
                packed, _ = ost.push(packed, ts=i, fmt=4)
                if packed is None:
                    continue
            out, _ = nd.deblock(packed, nd.FMT_YUV)
            want.append(np.concatenate([p.reshape(-1) for p in oracle.egress_obs("I420", out, planes=[np.full_like(p, 0x5A) for p in planes])]))
    r = subprocess.run([exe, "--stream", "1", str(rows), str(cols), str(n), str(delay), str(with_stab), str(tmp_path / "clip.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"stream ok: {len(want)} frames, region 0 0 480 256" in r.stdout, (r.stdout, r.stderr)
    assert len(want) == (n - delay if with_stab else n)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    assert got.size == sum(w.size for w in want)
    off = 0
    for i, w in enumerate(want):
        assert np.array_equal(got[off:off + w.size], w), i
        off += w.size
