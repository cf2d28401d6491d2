"""lvk::CASFilter of the C++ facade (include/lvk/CASFilter.hpp, driven by tests/cpp/cas_facade.cpp): apply against tests/np_cas.py, the
chain CompositeFilter{DeblockingFilter, CASFilter} against np_deblock followed by np_cas, and the OBS path (I420 through upload_obs_frame ->
apply -> download_ocl_frame) against the oracle's ingest / egress around np_cas.  CPU: it compiles and refuses a bad sharpness; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests import np_cas as nc
from tests.facade import build_facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cas_facade.cpp")


def _build(tmp_path):
    return build_facade(tmp_path, SRC, ["-pthread"])         # (the cross mode runs two threads)


def test_facade_cas_filter_compiles(tmp_path):
    _build(tmp_path)


def test_facade_configure_refuses_sharpness_outside_unit_interval(tmp_path):
    # configure({1.5}) and CASFilter({-0.25}) reach the assert handler; a refused configure keeps the settings (no device is touched)
    exe = _build(tmp_path)
    r = subprocess.run([exe, "configure"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "configure ok: 2 refused, alias CAS Filter" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,fmt,sharpness", [(270, 480, 0, 0.8), (131, 67, 4, 1.0), (1080, 1920, 2, 0.37), (1, 1, 4, 0.0)])
def test_facade_apply(tmp_path, rows, cols, fmt, sharpness):
    from tests.test_cas_gpu import content
    exe = _build(tmp_path)
    img = content(rows, cols, 3, seed=rows + cols)
    img.tofile(tmp_path / "frame.bin")
    r = subprocess.run([exe, "apply", str(fmt), str(rows), str(cols), repr(sharpness), str(tmp_path / "frame.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "apply ok: CAS Filter" in r.stdout, (r.stdout, r.stderr)
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.uint8).reshape(rows, cols, 3), nc.cas(img, sharpness))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,fmt,sharpness", [(270, 480, 4, 0.8), (1080, 1920, 0, 1.0)])
def test_facade_deblock_then_sharpen_chain(tmp_path, rows, cols, fmt, sharpness):
    from tests import np_deblock as nd
    from tests.test_deblock_gpu import blocky
    exe = _build(tmp_path)
    img = blocky(rows, cols, seed=rows + 3)
    img.tofile(tmp_path / "frame.bin")
    r = subprocess.run([exe, "chain", str(fmt), str(rows), str(cols), repr(sharpness), str(tmp_path / "frame.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "chain ok: Composite Filter" in r.stdout, (r.stdout, r.stderr)
    deblocked, _ = nd.deblock(img, fmt)
    assert not np.array_equal(deblocked, img)
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.uint8).reshape(rows, cols, 3), nc.cas(deblocked, sharpness))


@pytest.mark.gpu
def test_facade_two_contexts_feeding_each_other_from_two_threads(tmp_path):
    # the cross-context fences take both contexts' locks: taken under a filter's own lock they deadlock two filters that feed each other
    exe = _build(tmp_path)
    r = subprocess.run([exe, "cross", "0.8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cross ok" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.gpu
def test_facade_obs_i420_path(tmp_path, oracle):
    from tests import synth
    exe = _build(tmp_path)
    rows, cols, n, sharpness = 270, 480, 4, 0.8
    clip, _ = synth.make_clip(rows, cols, n, seed=67, jitter=1.0)
    want = []
    with open(tmp_path / "clip.bin", "wb") as f:
        for fr in clip:
            planes = oracle.egress_obs("I420", fr)
            for p in planes:
                f.write(p.tobytes())
            out = nc.cas(oracle.ingest_obs("I420", planes), sharpness)
            want.append(np.concatenate([p.reshape(-1) for p in oracle.egress_obs("I420", out, planes=[np.full_like(p, 0x5A) for p in planes])]))
    r = subprocess.run([exe, "--stream", "1", str(rows), str(cols), str(n), repr(sharpness), str(tmp_path / "clip.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"stream ok: {n} frames" in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    assert got.size == sum(w.size for w in want)
    off = 0
    for i, w in enumerate(want):
        assert np.array_equal(got[off:off + w.size], w), i
        off += w.size
