"""lvk::LCFilter of the C++ facade (include/lvk/LCFilter.hpp, tests/cpp/lc_filter_facade.cpp): a BGR frame, a GRAY frame and VideoFrame420 in both
layouts, the test mode, a size change on one filter and the filter inside CompositeFilter, against what this side computes from the oracle
(tests/lens_420_cases.py).  CPU: it compiles; GPU: it runs."""
import os
import subprocess

import numpy as np
import pytest

from tests.lens_420_cases import as_nv12, filter_expected, lens_map, oracle, packed_expected, packed_source, params_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lc_filter_facade.cpp")
SIZE, SIZE2 = (66, 130), (34, 66)
KIND = "smooth"


def test_facade_lc_filter_compiles(tmp_path):
    from tests.facade import build_facade
    build_facade(tmp_path, SRC)


def tight(planes):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])


def drive(tmp_path, mode, test_mode, profile, size, data, second=None):
    """Runs the program; returns the bytes it wrote (and those of the second size)."""
    from tests.facade import build_facade
    exe = build_facade(tmp_path, SRC)
    params = params_of(profile, *size)
    data.tofile(tmp_path / "in.bin")
    args = [exe, mode, str(int(test_mode)), "none" if params is None else ",".join(repr(v) for v in params), str(size[0]), str(size[1]),
            str(tmp_path / "in.bin"), str(tmp_path / "out.bin")]
    if second is not None:
        second[1].tofile(tmp_path / "in2.bin")
        args += [str(second[0][0]), str(second[0][1]), str(tmp_path / "in2.bin"), str(tmp_path / "out2.bin")]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lc filter ok: %s %dx%d" % (mode, size[1], size[0]) in r.stdout, (r.stdout, r.stderr)
    out = np.fromfile(tmp_path / "out.bin", np.uint8)
    return (out, np.fromfile(tmp_path / "out2.bin", np.uint8), r.stdout) if second is not None else (out, None, r.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("test_mode", [False, True], ids=["plain", "grid"])
@pytest.mark.parametrize("profile", [0, None], ids=["p0", "none"])
@pytest.mark.parametrize("mode", ["i420", "nv12"])
def test_facade_apply_420_with_a_size_change(tmp_path, mode, profile, test_mode):
    lay = as_nv12 if mode == "nv12" else tuple
    # one camera: the second, smaller frame is corrected with the profile of the first
    e, e2 = filter_expected(SIZE, profile, test_mode, KIND), filter_expected(SIZE2, profile, test_mode, KIND, at=SIZE)
    got, got2, stdout = drive(tmp_path, mode, test_mode, profile, SIZE, tight(lay(e["planes"])), (SIZE2, tight(lay(e2["planes"]))))
    assert np.array_equal(got, tight(lay(e["want"])))
    assert np.array_equal(got2, tight(lay(e2["want"])))
    assert "view %d %d %d %d" % e["view"] in stdout


@pytest.mark.gpu
@pytest.mark.parametrize("test_mode", [False, True], ids=["plain", "grid"])
@pytest.mark.parametrize("mode", ["bgr", "composite"])
def test_facade_bgr_frame_alone_and_inside_a_composite_filter(tmp_path, mode, test_mode):
    e = packed_expected(SIZE, 1, test_mode, False, KIND)
    got, _, _ = drive(tmp_path, mode, test_mode, 1, SIZE, np.ascontiguousarray(e["src"]).reshape(-1))
    assert np.array_equal(got.reshape(e["want"].shape), e["want"])


@pytest.mark.gpu
def test_facade_gray_frame(tmp_path):
    # the one-channel remap is channel 0 of the non-YUV program on (g, c, c)
    rows, cols = SIZE
    g = packed_source(rows, cols, KIND)[..., 0]
    want = oracle().remap_map(np.stack([g, np.full_like(g, 77), np.full_like(g, 77)], axis=2), lens_map(0, rows, cols)[0], bg=(0, 0, 0), yuv=False)[..., 0]
    got, _, _ = drive(tmp_path, "gray", False, 0, SIZE, np.ascontiguousarray(g).reshape(-1))
    assert np.array_equal(got.reshape(rows, cols), want)
