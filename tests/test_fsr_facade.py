"""lvk::FSRFilter of the C++ facade (include/lvk/FSRFilter.hpp, driven by tests/cpp/fsr_facade.cpp): apply in each settings mode against
tests/np_fsr.py, the chain CompositeFilter{FSRFilter, CASFilter} against np_fsr followed by np_cas, and the OBS path (I420 through
upload_obs_frame -> apply -> download_ocl_frame into an output-sized frame) against the oracle's ingest / egress around np_fsr.  CPU: it
compiles and refuses bad settings; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests import np_cas as nc
from tests import np_fsr as nf
from tests.facade import build_facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fsr_facade.cpp")


def test_facade_fsr_filter_compiles(tmp_path):
    build_facade(tmp_path, SRC)


def test_facade_configure_refuses_bad_settings(tmp_path):
    # negative or > 4096 crops, a multiplier <= 0 or NaN, a negative size reach the assert handler; a refused configure keeps the settings
    exe = build_facade(tmp_path, SRC)
    r = subprocess.run([exe, "configure"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "configure ok: 7 refused, alias FSR Filter" in r.stdout, (r.stdout, r.stderr)


# (fmt, rows, cols, out_size (rows, cols) or None, multiplier, aspect, crop)
MODES = [
    (0, 270, 480, None, 2.0, True, (0, 0, 0, 0)),                 # source x multiplier
    (4, 131, 67, None, 0.5, False, (0, 0, 0, 0)),
    (1, 270, 480, (400, 1000), 1.0, True, (0, 0, 0, 0)),          # explicit size, aspect fit
    (3, 270, 480, (400, 1000), 1.0, False, (10, 5, 30, 0)),       # explicit size, crop
    (2, 270, 480, None, 1.0, True, (0, 0, 0, 0)),                 # pass-through
    (0, 1, 1, (1, 1), 1.0, True, (0, 0, 0, 0)),
]


def _run(exe, tmp_path, mode, args):
    fmt, rows, cols, out_size, m, aspect, crop = args
    from tests.test_cas_gpu import content
    img = content(rows, cols, nf.CHANNELS[fmt], seed=rows + cols)
    img.tofile(tmp_path / "frame.bin")
    oh, ow = (0, 0) if out_size is None else out_size
    r = subprocess.run([exe, mode, str(fmt), str(rows), str(cols), str(oh), str(ow), repr(m), str(int(aspect)), *(str(c) for c in crop),
                        str(tmp_path / "frame.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    return img, r


@pytest.mark.gpu
@pytest.mark.parametrize("args", MODES)
def test_facade_apply(tmp_path, args):
    exe = build_facade(tmp_path, SRC)
    img, r = _run(exe, tmp_path, "apply", args)
    fmt, rows, cols, out_size, m, aspect, crop = args
    want = nf.fsr_filter(img, fmt, out_size, m, aspect, crop)
    assert r.returncode == 0 and "apply ok: FSR Filter" in r.stdout and r.stdout.split()[-1] == f"{want.shape[0]}x{want.shape[1]}", (r.stdout, r.stderr)
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.uint8).reshape(want.shape), want)


@pytest.mark.gpu
@pytest.mark.parametrize("args", [MODES[0], MODES[2], MODES[3]])
def test_facade_scale_then_sharpen_chain(tmp_path, args):
    exe = build_facade(tmp_path, SRC)
    img, r = _run(exe, tmp_path, "chain", args)
    fmt, rows, cols, out_size, m, aspect, crop = args
    want = nc.cas(nf.fsr_filter(img, fmt, out_size, m, aspect, crop), 0.8)
    assert r.returncode == 0 and "chain ok: Composite Filter" in r.stdout and r.stdout.split()[-1] == f"{want.shape[0]}x{want.shape[1]}", (r.stdout, r.stderr)
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.uint8).reshape(want.shape), want)


@pytest.mark.gpu
def test_facade_obs_i420_path(tmp_path, oracle):
    from tests import synth
    exe = build_facade(tmp_path, SRC)
    rows, cols, n, m = 270, 480, 3, 2.0
    clip, _ = synth.make_clip(rows, cols, n, seed=71, jitter=1.0)
    want = []
    with open(tmp_path / "clip.bin", "wb") as f:
        for fr in clip:
            planes = oracle.egress_obs("I420", fr)
            for p in planes:
                f.write(p.tobytes())
            out = nf.fsr_filter(oracle.ingest_obs("I420", planes), nf.FMT_YUV, None, m)
            blank = [np.full(sh, 0x5A, np.uint8) for sh in oracle.obs_plane_shapes("I420", out.shape[0], out.shape[1])]
            want.append(np.concatenate([p.reshape(-1) for p in oracle.egress_obs("I420", out, planes=blank)]))
    r = subprocess.run([exe, "--stream", "1", str(rows), str(cols), str(n), repr(m), str(tmp_path / "clip.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"stream ok: {n} frames 540x960" in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    assert got.size == sum(w.size for w in want)
    off = 0
    for i, w in enumerate(want):
        assert np.array_equal(got[off:off + w.size], w), i
        off += w.size
