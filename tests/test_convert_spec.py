"""CPU pins of the format conversion specification (tests/np_convert.py) and of its C-ABI surface.

The restatement is held to independent statements: the float64 textbook BT.601 YUV and its inverse over every 8-bit triple (observed
maxima pinned as literals), the tracker's own grey (the CPU oracle), PIL's ITU-R 601-2 luma, flat-colour literals, and the dispatch of
VideoFrame::reformatTo.  The conversion-code table comes from the built library (lvk_hip_cvt_code_target needs no device)."""
import os
import re

import numpy as np
import pytest

from tests import np_convert as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGR, BGRA, RGB, RGBA, YUV, GRAY = nc.FORMATS


def _all_triples():
    a = np.arange(1 << 24, dtype=np.int32)
    return a & 255, (a >> 8) & 255, a >> 16


# ---- closed-form bounds over every triple -------------------------------------------------------------------------------------------

def test_yuv_is_within_one_lsb_of_the_textbook_over_every_triple():
    b, g, r = _all_triples()
    y, u, v = nc.yuv_of(b, g, r)
    Y = 0.299 * r + 0.587 * g + 0.114 * b
    U = np.clip(0.492 * (b - Y) + 128, 0, 255)
    V = np.clip(0.877 * (r - Y) + 128, 0, 255)
    ey, eu, ev = (float(np.abs(p - q).max()) for p, q in ((y, Y), (u, U), (v, V)))
    assert max(ey, eu, ev) < 1.0
    assert (round(ey, 3), round(eu, 3), round(ev, 3)) == (0.506, 0.745, 0.937)


def test_inverse_is_within_one_lsb_of_the_textbook_over_every_triple():
    y, u, v = _all_triples()
    b, g, r = nc.bgr_of_yuv(y, u, v, saturate=False)
    du, dv = u - 128.0, v - 128.0
    B, G, R = y + 2.032 * du, y - 0.395 * du - 0.581 * dv, y + 1.140 * dv
    eb, eg, er = (float(np.abs(p - q).max()) for p, q in ((b, B), (g, G), (r, R)))
    assert max(eb, eg, er) < 1.0
    assert (round(eb, 3), round(eg, 3), round(er, 3)) == (0.496, 0.502, 0.5)


def test_round_trip_maxima_over_every_triple():
    # U and V saturate on strong colours, so BGR -> YUV -> BGR loses up to 17 (G) and 34 (R) levels; pure red is such a colour
    b, g, r = _all_triples()
    b2, g2, r2 = nc.bgr_of_yuv(*nc.yuv_of(b, g, r))
    assert (int(np.abs(b2 - b).max()), int(np.abs(g2 - g).max()), int(np.abs(r2 - r).max())) == (1, 17, 34)
    red = nc.reformat(np.array([[[0, 0, 255]]], np.uint8), BGR, YUV)
    assert red.tolist() == [[[76, 91, 255]]]
    assert nc.reformat(red, YUV, BGR).tolist() == [[[1, 17, 221]]]


def test_gray_is_within_one_lsb_of_pil_over_every_triple():
    from PIL import Image
    b, g, r = _all_triples()
    rgb = np.stack([r, g, b], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    pil = np.asarray(Image.fromarray(rgb, "RGB").convert("L")).reshape(-1).astype(np.int32)
    ours = nc.gray_of(b, g, r)
    assert int(np.abs(ours - pil).max()) == 1
    assert np.array_equal(nc.reformat(rgb, RGB, GRAY)[..., 0].reshape(-1), ours)


def test_gray_is_the_trackers_gray(oracle):
    # the tracker's luma (oracle/imgproc.cpp: cvtColor BGR2GRAY / RGB2GRAY, then INTER_AREA) at identity size is the grey itself
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    assert np.array_equal(oracle.luma_area_resize(img, 64, 96, channel=-1), nc.reformat(img, BGR, GRAY)[..., 0])
    assert np.array_equal(oracle.luma_area_resize(img, 64, 96, channel=-2), nc.reformat(img, RGB, GRAY)[..., 0])


# ---- the 30 pairs -------------------------------------------------------------------------------------------------------------------

WHITE, BLACK, BLUE, GREEN, RED = (255, 255, 255), (0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)     # as BGR


def _bgr_frame(*colours):
    return np.array([list(colours)], np.uint8)


def test_every_pair_is_dispatched():
    pairs = {(s, d) for s in nc.FORMATS for d in nc.FORMATS if s != d}
    assert len(pairs) == 30 and set(nc.PAIRS) == pairs


def test_flat_colour_literals():
    img = _bgr_frame(WHITE, BLACK, BLUE, GREEN, RED)
    assert nc.reformat(img, BGR, YUV).tolist() == [[[255, 128, 128], [0, 128, 128], [29, 239, 103], [150, 54, 0], [76, 91, 255]]]
    assert nc.reformat(img, BGR, GRAY)[..., 0].tolist() == [[255, 0, 29, 150, 76]]
    assert nc.reformat(img, RGB, GRAY)[..., 0].tolist() == [[255, 0, 76, 150, 29]]
    assert nc.reformat(img, BGR, RGBA).tolist() == [[[255, 255, 255, 255], [0, 0, 0, 255], [0, 0, 255, 255], [0, 255, 0, 255],
                                                     [255, 0, 0, 255]]]
    yuv = np.array([[[128, 128, 128], [255, 128, 128], [0, 128, 128], [76, 91, 255]]], np.uint8)
    assert nc.reformat(yuv, YUV, BGR).tolist() == [[[128, 128, 128], [255, 255, 255], [0, 0, 0], [1, 17, 221]]]
    assert nc.reformat(yuv, YUV, RGBA).tolist() == [[[128, 128, 128, 255], [255, 255, 255, 255], [0, 0, 0, 255], [221, 17, 1, 255]]]
    assert nc.reformat(yuv, YUV, GRAY)[..., 0].tolist() == [[128, 255, 0, 76]]
    gray = np.array([[[0], [77], [255]]], np.uint8)
    assert nc.reformat(gray, GRAY, YUV).tolist() == [[[0, 128, 128], [77, 128, 128], [255, 128, 128]]]
    assert nc.reformat(gray, GRAY, BGRA).tolist() == [[[0, 0, 0, 255], [77, 77, 77, 255], [255, 255, 255, 255]]]


def test_byte_shuffles_and_the_four_channel_two_step():
    rng = np.random.default_rng(3)
    bgra = rng.integers(0, 256, (7, 9, 4), dtype=np.uint8)
    bgr, rgb, rgba = bgra[..., :3], bgra[..., 2::-1], bgra[..., [2, 1, 0, 3]]
    assert np.array_equal(nc.reformat(bgra, BGRA, BGR), bgr)
    assert np.array_equal(nc.reformat(bgra, BGRA, RGB), rgb)
    assert np.array_equal(nc.reformat(bgra, BGRA, RGBA), rgba)
    assert np.array_equal(nc.reformat(rgba, RGBA, BGRA), bgra)
    assert np.array_equal(nc.reformat(bgr, BGR, BGRA)[..., 3], np.full((7, 9), 255, np.uint8))     # 3 -> 4 writes 255, 4 -> 4 keeps alpha
    # BGRA -> YUV is BGRA2BGR then BGR2YUV (VideoFrame.cpp:212-216), RGBA -> YUV likewise; GRAY of 4 channels ignores alpha
    assert np.array_equal(nc.reformat(bgra, BGRA, YUV), nc.reformat(nc.reformat(bgra, BGRA, BGR), BGR, YUV))
    assert np.array_equal(nc.reformat(rgba, RGBA, YUV), nc.reformat(nc.reformat(rgba, RGBA, RGB), RGB, YUV))
    assert np.array_equal(nc.reformat(bgra, BGRA, GRAY), nc.reformat(bgr, BGR, GRAY))
    # the same format on both sides is a copy
    out = nc.reformat(bgra, BGRA, BGRA)
    assert np.array_equal(out, bgra) and out is not bgra


# ---- the conversion-code table ------------------------------------------------------------------------------------------------------

def test_code_table_of_the_library_is_the_specification():
    from livevisionkit_amd import _native
    lib = _native.load()
    accepted = 0
    for code in range(151):
        for fmt in list(nc.FORMATS) + [-1, 6, 99]:
            for dcn in range(5):
                want = nc.code_target(code, fmt, dcn) if fmt in nc.FORMATS else -1
                assert lib.lvk_hip_cvt_code_target(code, fmt, dcn) == want, (code, fmt, dcn)
                accepted += want >= 0
    assert accepted == 12 * 2 * 2 + 2 * 2 + 2 * 3     # (format, dcn): 12 codes take 2 formats x dcn {0, own}; GRAY2* 1 x 2; YUV2* 1 x {0, 3, 4}


@pytest.mark.parametrize("code,fmt,dcn,want", [
    (nc.COLOR_BGR2YUV, BGRA, 0, YUV), (nc.COLOR_RGB2YUV, RGBA, 3, YUV), (nc.COLOR_BGR2YUV, RGB, 0, -1),
    (nc.COLOR_YUV2BGR, YUV, 4, BGRA), (nc.COLOR_YUV2RGB, YUV, 4, RGBA), (nc.COLOR_YUV2RGB, YUV, 1, -1), (nc.COLOR_YUV2BGR, BGR, 0, -1),
    (nc.COLOR_RGB2RGBA, RGB, 4, RGBA), (nc.COLOR_BGR2BGRA, BGR, 3, -1), (nc.COLOR_BGRA2RGB, BGRA, 0, RGB), (nc.COLOR_RGBA2BGR, RGBA, 0, BGR),
    (nc.COLOR_BGR2GRAY, BGRA, 1, GRAY), (nc.COLOR_RGBA2GRAY, RGB, 0, GRAY), (nc.COLOR_RGBA2GRAY, BGRA, 0, -1),
    (nc.COLOR_GRAY2RGB, GRAY, 0, BGR), (nc.COLOR_GRAY2BGRA, GRAY, 4, BGRA), (nc.COLOR_GRAY2BGRA, YUV, 0, -1),
    (40, BGR, 0, -1), (127, YUV, 0, -1), (-1, BGR, 0, -1)])          # BGR2HSV, YUV2RGB_I420: not taken
def test_code_table_literals(code, fmt, dcn, want):
    from livevisionkit_amd.convert import code_target
    assert nc.code_target(code, fmt, dcn) == want
    assert code_target(code, fmt, dcn) == want


# ---- the C-ABI surface --------------------------------------------------------------------------------------------------------------

def test_header_declares_the_conversion_abi():
    text = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    assert re.search(r"int\s+lvk_hip_reformat\(lvk_hip_ctx\* ctx, const void\* d_src, int src_step, int rows, int cols, int src_format,\s+"
                     r"void\* d_dst, int dst_step,\s+int dst_format\);", stable)
    assert "lvk_hip_reformat(" not in experimental
    assert "int lvk_hip_cvt_code_target(int code, int src_format, int dcn);" in experimental and "lvk_hip_cvt_code_target(" not in stable
    assert int(re.search(r"#define LVK_HIP_ABI_VERSION (\d+)", text).group(1)) >= 9


def test_library_reports_abi_9_and_refuses_without_a_context():
    from livevisionkit_amd import _native
    lib = _native.load()
    assert lib.lvk_hip_abi_version() >= 9
    assert b"ABI %d" % lib.lvk_hip_abi_version() in lib.lvk_hip_version()
    assert lib.lvk_hip_reformat(None, None, 3, 1, 1, BGR, None, 3, YUV) != 0


def test_python_binding_is_exported():
    import livevisionkit_amd as lvk
    assert "ConversionFilter" in lvk.__all__ and "reformat" in lvk.__all__
    from livevisionkit_amd import convert
    assert convert.COLOR_BGR2YUV == 82 and convert.COLOR_YUV2RGB == 85 and convert.COLOR_RGBA2BGR == convert.COLOR_BGRA2RGB == 3
    assert convert.CHANNELS == {k: v for k, v in nc.CHANNELS.items()}


def test_python_filter_refuses_unsupported_codes_without_a_device():
    from livevisionkit_amd.convert import ConversionFilter
    with pytest.raises(ValueError):
        ConversionFilter(None, 40)                         # BGR2HSV
    with pytest.raises(ValueError):
        ConversionFilter(None, nc.COLOR_BGR2YUV, output_channels=4)
    f = ConversionFilter(None, nc.COLOR_YUV2BGR, output_channels=4)
    assert f.target(YUV) == BGRA
    with pytest.raises(ValueError):
        f.target(BGR)
