"""The premises of the one- and four-channel EASU upscale and RCAS, on the CPU.

The reference's lvk::upscale and lvk::sharpen assert CV_8UC3, so both operations are DEFINED for these frames through the three-channel programs
(tests/scaling_px_cases.py evaluates the definitions).  They are definitions only if
  1. output channel k of the non-YUV easu_scale program depends on input channels 0 and k alone (GRAY: channel 0 of (g, c, c) for ANY c; four channels: the
     alpha as channel 1 of (c0, a, a)), which the YUV program does not do;
  2. the rcas program of (g, g, g) has three equal channels (GRAY: "any channel"), while its channels ARE coupled in general -- which is why alpha cannot
     ride along as a fourth channel of the limiter without changing the colours, and is copied.
These tests pin both for the oracle and for its numpy twin.  The last test holds the C ABI: the four symbols are declared, exported and bound."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import np_easu
from tests.scaling_px_cases import frame, saturate_rings, sharpen_gray, upscale_c4, upscale_gray, with_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["lvk_hip_upscale_gray", "lvk_hip_upscale_c4", "lvk_hip_sharpen_gray", "lvk_hip_sharpen_c4"]
UPSCALES = [((8, 8), (9, 8)), ((9, 11), (23, 17)), ((21, 34), (64, 49)), ((41, 57), (100, 83))]         # (rows, cols) -> (width, height)
SHARPEN_SIZES = [(3, 3), (5, 9), (17, 33), (41, 57)]
SHARPNESS = [0.0, 0.8, 1.0]


def _upscales(oracle, yuv):
    return [("oracle", lambda f, size: oracle.upscale(f, size, yuv=yuv)), ("numpy", lambda f, size: np_easu.upscale(f, size, yuv))]


def _sharpens(oracle):
    return [("oracle", oracle.sharpen), ("numpy", np_easu.sharpen)]


@pytest.mark.parametrize("src_size,dst_size", UPSCALES)
def test_output_channel_k_of_the_non_yuv_upscale_depends_on_input_channels_0_and_k_only(oracle, src_size, dst_size):
    rows, cols = src_size
    c0, c1, c2, a = (frame(rows, cols)[..., k] for k in range(4))
    rnd = np.random.default_rng(9).integers(0, 256, (rows, cols), dtype=np.uint8)
    zero = np.zeros_like(a)
    for name, up in _upscales(oracle, False):
        # GRAY: channel 0 of (g, c, c) is the same for every c, and for planes that are no constants
        grays = [upscale_gray(up, c0, dst_size, c) for c in (0, 128, 255)] + [up(with_(c0, rnd, a), dst_size)[..., 0]]
        assert all(np.array_equal(grays[0], g) for g in grays[1:]), name
        assert grays[0].shape == (dst_size[1], dst_size[0])
        # byte 3 of four channels: channel 1 of (c0, a, a) = of (c0, a, 0) = of (c0, a, random) -- the kernels run the core on (c0, a, 0)
        alphas = [up(with_(c0, a, third), dst_size)[..., 1] for third in (a, zero, rnd)]
        assert np.array_equal(alphas[0], alphas[1]) and np.array_equal(alphas[0], alphas[2]), name
        assert np.array_equal(upscale_c4(up, frame(rows, cols), dst_size)[..., 3], alphas[0]), name
        # bytes 0 and 2 of (c0, c1, c2) do not change when channel 1 is replaced
        base = up(with_(c0, c1, c2), dst_size)
        for other in (a, zero, rnd):
            got = up(with_(c0, other, c2), dst_size)
            assert np.array_equal(got[..., 0], base[..., 0]) and np.array_equal(got[..., 2], base[..., 2]), name
        # ... and the test can tell: channel 1 itself follows its input
        assert not np.array_equal(up(with_(c0, rnd, c2), dst_size)[..., 1], base[..., 1]), name


def test_the_yuv_upscale_fails_the_same_test(oracle):
    """Its luma mixes the three channels, so its weights -- and every output channel -- depend on all of them: the definitions name the non-YUV program."""
    (rows, cols), dst_size = UPSCALES[-1]
    c0, c1, c2, a = (frame(rows, cols)[..., k] for k in range(4))
    rnd = np.random.default_rng(9).integers(0, 256, (rows, cols), dtype=np.uint8)
    for name, up in _upscales(oracle, True):
        assert not np.array_equal(up(with_(c0, a, a), dst_size)[..., 1], up(with_(c0, a, rnd), dst_size)[..., 1]), name
        assert not np.array_equal(up(with_(c0, c1, c2), dst_size)[..., 0], up(with_(c0, rnd, c2), dst_size)[..., 0]), name


@pytest.mark.parametrize("sharpness", SHARPNESS)
@pytest.mark.parametrize("size", SHARPEN_SIZES)
def test_rcas_of_a_grey_frame_has_three_equal_channels(oracle, size, sharpness):
    """... rings saturated at 0 and at 255 included, where a limiter is the NaN of 0 x inf and loses against -0.1875 in every channel alike."""
    g = saturate_rings(frame(*size)[..., 0].copy())
    for name, sh in _sharpens(oracle):
        out = sh(with_(g, g, g), sharpness)
        assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2]), name
        assert np.array_equal(sharpen_gray(sh, g, sharpness), out[..., 1]), name
        # border pixels are copied
        assert np.array_equal(out[0], with_(g, g, g)[0]) and np.array_equal(out[:, -1], with_(g, g, g)[:, -1]), name
    if min(size) >= 5 and sharpness > 0:                      # ... and the test can tell: the interior is sharpened
        assert not np.array_equal(oracle.sharpen(with_(g, g, g), sharpness), with_(g, g, g))


@pytest.mark.parametrize("size", [s for s in SHARPEN_SIZES if s != (3, 3)])
def test_rcas_channels_are_coupled(oracle, size):
    """The three lobes meet in one maximum (FSR.cl:525): channel 0 of the output changes with channel 1 of the input.  A fourth channel in the limiter would
    change the colours, so the four-channel definition leaves alpha out of it."""
    c0, c1, c2, _ = (saturate_rings(frame(*size))[..., k] for k in range(4))
    rnd = np.random.default_rng(9).integers(0, 256, size, dtype=np.uint8)          # (a plane of high contrast: its lobe is the maximum at many pixels)
    for name, sh in _sharpens(oracle):
        assert not np.array_equal(sh(with_(c0, c1, c2), 0.8)[..., 0], sh(with_(c0, rnd, c2), 0.8)[..., 0]), name


def test_the_library_exports_and_the_header_declares_the_four_entries():
    header = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "livevisionkit_amd", "liblvk_hip.so"))
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} is not declared in include/lvk_hip.h"
        assert hasattr(lib, sym), f"{sym} is not exported by liblvk_hip.so"
    from livevisionkit_amd import _native
    assert all(sym in _native._SIG for sym in SYMBOLS)
    import livevisionkit_amd as lvk
    assert all(hasattr(lvk.Context, m) for m in ("upscale_gray", "upscale_c4", "sharpen_gray", "sharpen_c4"))
