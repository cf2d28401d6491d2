"""VideoFrame::reformat / reformatTo / viewAsFormat and lvk::ConversionFilter of the C++ facade (driven by tests/cpp/convert_facade.cpp):
1-, 3- and 4-channel frames, the 36 format pairs through the three VideoFrame calls, every ConversionFilter code against tests/np_convert.py,
the chain CompositeFilter{ConversionFilter(YUV2BGR), CASFilter, ConversionFilter(BGR2YUV)} against np_convert around np_cas, and the
plugin's export step (I420 through upload_obs_frame, then viewAsFormat(RGBA)) against the oracle's ingest followed by np_convert.
CPU: it compiles and refuses unsupported codes; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests import np_convert as nc
from tests.facade import build_facade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "convert_facade.cpp")


def _inputs(tmp_path, rows, cols, seed):
    rng = np.random.default_rng(seed)
    imgs = {}
    for f in nc.FORMATS:
        imgs[f] = rng.integers(0, 256, (rows, cols, nc.CHANNELS[f]), dtype=np.uint8)
        imgs[f].tofile(tmp_path / ("in_%d.bin" % f))
    return imgs


def _read(path, rows, cols, fmt):
    return np.fromfile(path, np.uint8).reshape(rows, cols, nc.CHANNELS[fmt])


def test_facade_conversion_filter_compiles(tmp_path):
    build_facade(tmp_path, SRC)


def test_facade_configure_refuses_unsupported_codes(tmp_path):
    # unsupported codes and output channels reach the assert handler; a refused configure keeps the settings (no device is touched)
    exe = build_facade(tmp_path, SRC)
    r = subprocess.run([exe, "configure"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "configure ok: 6 refused, alias Conversion Filter" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(1, 1), (17, 65), (270, 480)])
def test_facade_frames_of_one_three_and_four_channels(tmp_path, rows, cols):
    exe = build_facade(tmp_path, SRC)
    r = subprocess.run([exe, "frames", str(rows), str(cols)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "frames ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(3, 5), (31, 67), (1080, 1920)])
def test_facade_reformat_reformat_to_and_view_as_format(tmp_path, rows, cols):
    exe = build_facade(tmp_path, SRC)
    imgs = _inputs(tmp_path, rows, cols, seed=rows + cols)
    r = subprocess.run([exe, "reformat", str(rows), str(cols), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "reformat ok: 36 pairs" in r.stdout, (r.returncode, r.stdout, r.stderr)
    for s in nc.FORMATS:
        for d in nc.FORMATS:
            want = nc.reformat(imgs[s], s, d)
            for kind in ("to", "re", "view"):
                got = _read(tmp_path / ("%s_%d_%d.bin" % (kind, s, d)), rows, cols, d)
                assert np.array_equal(got, want), (kind, nc.NAMES[s], nc.NAMES[d])


@pytest.mark.gpu
def test_facade_conversion_filter_every_code(tmp_path):
    rows, cols = 45, 83
    exe = build_facade(tmp_path, SRC)
    imgs = _inputs(tmp_path, rows, cols, seed=9)
    r = subprocess.run([exe, "filter", str(rows), str(cols), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "filter ok:" in r.stdout and "Conversion Filter" in r.stdout, (r.returncode, r.stdout, r.stderr)
    cases = [tuple(map(int, line.split()[1:])) for line in r.stdout.splitlines() if line.startswith("cf ")]
    # every code with each source format it takes, without output_channels and with 4 where the code takes it (YUV2BGR / YUV2RGB too)
    want_cases = {(code, s, dcn) for code in nc.CODES for s in nc.FORMATS for dcn in (0, 4) if nc.code_target(code, s, dcn) >= 0}
    assert {c[:3] for c in cases} == want_cases and len(cases) == len(want_cases) == 37
    for code, s, dcn, to in cases:
        want, want_to = nc.convert(imgs[s], s, code, dcn)
        assert to == want_to, (code, s, dcn)
        assert np.array_equal(_read(tmp_path / ("cf_%d_%d_%d.bin" % (code, s, dcn)), rows, cols, to), want), (code, s, dcn)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,sharpness", [(270, 480, 0.8), (1080, 1920, 1.0)])
def test_facade_yuv_to_bgr_sharpen_and_back_chain(tmp_path, rows, cols, sharpness):
    from tests import np_cas
    from tests.test_cas_gpu import content
    exe = build_facade(tmp_path, SRC)
    img = content(rows, cols, 3, seed=rows + 11)
    img.tofile(tmp_path / "frame.bin")
    r = subprocess.run([exe, "chain", str(rows), str(cols), repr(sharpness), str(tmp_path / "frame.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "chain ok: Composite Filter" in r.stdout, (r.returncode, r.stdout, r.stderr)
    want = nc.reformat(np_cas.cas(nc.reformat(img, nc.YUV, nc.BGR), sharpness), nc.BGR, nc.YUV)
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.uint8).reshape(rows, cols, 3), want)


@pytest.mark.gpu
def test_facade_obs_i420_export_as_rgba(tmp_path, oracle):
    from tests import synth
    exe = build_facade(tmp_path, SRC)
    rows, cols, n = 270, 480, 3
    clip, _ = synth.make_clip(rows, cols, n, seed=71, jitter=1.0)
    want = []
    with open(tmp_path / "clip.bin", "wb") as f:
        for fr in clip:
            planes = oracle.egress_obs("I420", fr)
            for p in planes:
                f.write(p.tobytes())
            want.append(nc.reformat(oracle.ingest_obs("I420", planes), nc.YUV, nc.RGBA))
    r = subprocess.run([exe, "--stream", str(rows), str(cols), str(n), str(tmp_path / "clip.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"stream ok: {n} frames" in r.stdout, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(n, rows, cols, 4)
    for i, w in enumerate(want):
        assert np.array_equal(got[i], w), i
