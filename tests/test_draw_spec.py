"""The specification of the device drawing calls (tests/np_draw.py) against answers written out by hand, the host-only lvk_hip_text_size against
it, and the ABI surface of the three calls.  No GPU needed: the kernels are held to the same specification in tests/test_draw_suite_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import np_draw as nd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLOUR = (7, 200, 99)


def _art(text):
    """A boolean mask from rows of '#' and '.'."""
    rows = text.split()
    assert len({len(r) for r in rows}) == 1
    return np.array([[c == "#" for c in r] for r in rows], dtype=bool)


def _drawn(before, after):
    """The mask of the pixels that were drawn; checks that they carry COLOUR and that nothing else changed."""
    changed = (before != after).any(axis=2)
    assert (after[changed] == COLOUR).all()
    return changed


def _blank(rows, cols):
    return np.zeros((rows, cols, 3), np.uint8)


# ---- rectangles -------------------------------------------------------------------------------------------------------------------------
def test_rect_one_pixel_outline():
    want = _art("""
        .........
        ..#####..
        ..#...#..
        ..#...#..
        ..#####..
        .........
        .........""")
    img = _blank(7, 9)
    assert np.array_equal(_drawn(img, nd.rect(img, (2, 1, 5, 4), COLOUR, 1)), want)
    assert np.array_equal(nd.rect_mask(7, 9, (2, 1, 5, 4), 1), want)


def test_rect_band_of_two():
    # a = 1, b = 0: one pixel outwards at the top-left corner (x0 - 1, y0 - 1), one inwards at the bottom-right one
    want = _art("""
        .######..
        .######..
        .##..##..
        .######..
        .######..
        .........
        .........""")
    assert np.array_equal(nd.rect_mask(7, 9, (2, 1, 5, 4), 2), want)


def test_rect_band_of_three():
    # a = b = 1: the outline with one pixel on either side of it; square corners
    want = _art("""
        ..........
        .########.
        .########.
        .########.
        .###..###.
        .########.
        .########.
        .########.
        ..........""")
    assert np.array_equal(nd.rect_mask(9, 10, (2, 2, 6, 5), 3), want)


def test_rect_filled():
    want = _art("""
        ......
        ......
        .###..
        .###..
        ......""")
    img = _blank(5, 6)
    assert np.array_equal(_drawn(img, nd.rect(img, (1, 2, 3, 2), COLOUR, -1)), want)
    assert np.array_equal(nd.rect_mask(5, 6, (1, 2, 3, 2), -7), want)              # any negative thickness


def test_rect_clipped_at_each_edge():
    top_left = _art("""
        ..#...
        ..#...
        ###...
        ......
        ......""")
    assert np.array_equal(nd.rect_mask(5, 6, (-2, -1, 5, 4), 1), top_left)
    bottom_right = _art("""
        ......
        ......
        ......
        ....##
        ....#.""")
    assert np.array_equal(nd.rect_mask(5, 6, (4, 3, 5, 5), 1), bottom_right)
    top = _art("""
        .#..#.
        .####.
        ......
        ......
        ......""")
    assert np.array_equal(nd.rect_mask(5, 6, (1, -3, 4, 5), 1), top)
    bottom = _art("""
        ......
        ......
        ......
        .####.
        .#..#.""")
    assert np.array_equal(nd.rect_mask(5, 6, (1, 3, 4, 5), 1), bottom)
    left = _art("""
        ......
        ##....
        .#....
        ##....
        ......""")
    assert np.array_equal(nd.rect_mask(5, 6, (-3, 1, 5, 3), 1), left)
    right = _art("""
        ......
        ....##
        ....#.
        ....##
        ......""")
    assert np.array_equal(nd.rect_mask(5, 6, (4, 1, 5, 3), 1), right)
    band_over_the_top = _art("""
        ##..##
        ##..##
        ######
        ######
        ......""")
    assert np.array_equal(nd.rect_mask(5, 6, (1, -2, 5, 6), 2), band_over_the_top)   # x 0 .. 5, y -3 .. 3; hole x 2 .. 3, y -1 .. 1
    assert not nd.rect_mask(5, 6, (-1, -1, 8, 7), 1).any()                          # the frame lies inside the outline
    assert not nd.rect_mask(5, 6, (10, 10, 3, 3), 3).any() and not nd.rect_mask(5, 6, (-9, 0, 3, 3), -1).any()
    assert nd.rect_mask(5, 6, (-1, -1, 8, 7), -1).all()


# ---- points -----------------------------------------------------------------------------------------------------------------------------
def test_points_at_the_first_pixel_and_past_the_last():
    want = _art("""
        ##....
        ##....
        ......
        ....##
        ....##""")
    img = _blank(5, 6)
    assert np.array_equal(_drawn(img, nd.points(img, [(0, 0), (6, 5)], COLOUR, 3)), want)          # half width (3 + 1) / 2 = 2
    assert np.array_equal(_drawn(img, nd.points(img, [(0, 0), (6, 5)], COLOUR, 4)), want)          # (4 + 1) / 2 = 2
    one = _art("""
        ......
        ..##..
        ..##..
        ......
        ......""")
    assert np.array_equal(_drawn(img, nd.points(img, [(3, 2)], COLOUR, 1)), one)                   # [px - 1, px + 1)
    assert np.array_equal(_drawn(img, nd.points(img, [(1.5, 0.5)], COLOUR, 1, scaling=(2.0, 4.0))), one)   # 3.0, 2.0
    assert np.array_equal(nd.scale_points([(0.5, 1.5), (2.5, -0.5), (np.nan, 1e20)]), [[0, 2], [2, 0], [0, 2 ** 30]])   # half to even
    assert np.array_equal(nd.points(img, np.zeros((0, 2)), COLOUR, 3), img)
    assert np.array_equal(nd.points(img, [(-40, 2), (3, 90)], COLOUR, 9), img)


# ---- text -------------------------------------------------------------------------------------------------------------------------------
def test_font_table_is_well_formed():
    assert len(nd.FONT) == 95
    for i, g in enumerate(nd.FONT):
        rows = g.split("/")
        assert len(rows) == nd.GLYPH_H and all(len(r) == nd.GLYPH_W and set(r) <= set("#.") for r in rows), chr(0x20 + i)
    assert not nd.glyph(0x20).any()
    assert all(nd.glyph(b).any() for b in range(0x21, 0x7F))
    assert len({nd.FONT[i] for i in range(1, 95)}) >= 92            # glyphs are told apart (O and 0, I and l may not coincide either)
    assert nd.FONT[ord("O") - 0x20] != nd.FONT[ord("0") - 0x20] and nd.FONT[ord("I") - 0x20] != nd.FONT[ord("l") - 0x20]
    for b in (0x01, 0x1F, 0x7F, 0x80, 0xFF):
        assert np.array_equal(nd.glyph(b), nd.glyph(ord("?")))


def test_text_letter_by_hand():
    # 'L' at scale 2: every font pixel a 2 x 2 block, the baseline's left end at (1, 15): rows 1 .. 14, columns 1 .. 10
    want = np.zeros((16, 12), bool)
    want[1:15, 1:3] = True
    want[13:15, 1:11] = True
    assert np.array_equal(nd.text_mask(16, 12, "L", (1, 15), 2, 1), want)
    assert np.array_equal(nd.text_mask(16, 12, "L", (1, 15), 2, 2), want)          # thickness 2 grows by (2 - 1) / 2 = 0
    grown = np.zeros((16, 12), bool)
    grown[0:16, 0:4] = True
    grown[12:16, 0:12] = True
    assert np.array_equal(nd.text_mask(16, 12, "L", (1, 15), 2, 3), grown)         # one pixel on each side


def test_hud_string_fills_its_text_size_and_counts_its_bits():
    s = "0.12ms (3.40ms)"
    (w, h), baseline = nd.text_size(s, 1, 1)
    assert (w, h, baseline) == (6 * len(s) - 1, 7, 1)
    mask = nd.text_mask(20, 100, s, (3, 12), 1, 1)
    ys, xs = np.nonzero(mask)
    # '0' reaches the first column and both the top and the bottom row, ')' the last column: the drawn box is text_size, its bottom row y - 1
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (3, 3 + w - 1, 12 - h, 12 - 1)
    assert mask.sum() == sum(int(nd.glyph(b).sum()) for b in s.encode())
    img = np.full((20, 100, 3), 31, np.uint8)
    out = nd.text(img, s, (3, 12), COLOUR, 1, 1)
    assert np.array_equal(_drawn(img, out), mask)
    # clipped: the part inside the frame is the same picture
    assert np.array_equal(nd.text_mask(9, 40, s, (3 - 20, 12 - 4), 1, 1), mask[4:13, 20:60])
    assert not nd.text_mask(20, 100, "", (3, 12), 1, 1).any() and nd.text_size("", 4, 3) == ((0, 30), 5)
    assert not nd.text_mask(20, 100, s, (3, 0), 1, 1).any() and not nd.text_mask(20, 100, s, (100, 12), 1, 1).any()
    assert nd.font_scale_to_scale(1.5) == 3 and nd.font_scale_to_scale(0.1) == 1 and nd.font_scale_to_scale(1.25) == 2 and nd.font_scale_to_scale(0.75) == 2


def test_library_text_size_matches_the_specification():
    import livevisionkit_amd as lvk
    rng = np.random.default_rng(17)
    for _ in range(400):
        n = int(rng.choice([0, 1, 2, 15, 255, 256, int(rng.integers(0, 257))]))
        text = bytes(rng.integers(1, 256, n, dtype=np.uint8).tolist())
        scale, thickness = int(rng.integers(1, 41)), int(rng.integers(1, 10))
        assert lvk.text_size(text, scale, thickness) == nd.text_size(text, scale, thickness), (n, scale, thickness)
    assert lvk.text_size("0.12ms (3.40ms)") == nd.text_size("0.12ms (3.40ms)") == ((267, 21), 3)
    assert lvk.text_size("x", nd.MAX_SCALE, nd.MAX_THICKNESS) == nd.text_size("x", nd.MAX_SCALE, nd.MAX_THICKNESS)


def test_refused_calls():
    import livevisionkit_amd as lvk
    from livevisionkit_amd import _native
    for text, scale, thickness in (("a" * 257, 1, 1), ("a", 0, 1), ("a", 1, 0), ("a", -3, 1), ("a", 1, -1), ("a", nd.MAX_SCALE + 1, 1),
                                   ("a", 1, nd.MAX_THICKNESS + 1)):
        with pytest.raises(ValueError):
            nd.text_size(text, scale, thickness)
        with pytest.raises(ValueError):
            nd.text_mask(8, 8, text, (0, 7), scale, thickness)
        with pytest.raises(ValueError):
            lvk.text_size(text, scale, thickness)
    lib = _native.load()
    wh, baseline = (ctypes.c_int * 2)(5, 6), ctypes.c_int(7)
    assert lib.lvk_hip_text_size(None, 1, 1, wh, ctypes.byref(baseline)) == -1
    assert lib.lvk_hip_text_size(b"a", 1, 1, None, ctypes.byref(baseline)) == -1
    assert lib.lvk_hip_text_size(b"a", 1, 1, wh, None) == -1
    assert lib.lvk_hip_text_size(b"a" * 257, 1, 1, wh, ctypes.byref(baseline)) == -1
    assert (wh[0], wh[1], baseline.value) == (5, 6, 7)                  # a refused call writes nothing
    img = _blank(4, 4)
    for rect, thickness in (((0, 0, 2, 2), 0), ((0, 0, 0, 2), 1), ((0, 0, 2, -1), 1), ((1, 1, -2, 2), -1)):
        with pytest.raises(ValueError):
            nd.rect(img, rect, COLOUR, thickness)
    for size, scaling in ((0, (1, 1)), (-2, (1, 1)), (3, (-1.0, 1)), (3, (1, -0.5)), (3, (np.nan, 1))):
        with pytest.raises(ValueError):
            nd.points(img, [(1, 1)], COLOUR, size, scaling)
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32)):
        with pytest.raises(ValueError):
            nd.rect(bad, (0, 0, 2, 2), COLOUR, 1)


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------
def test_abi_surface():
    import livevisionkit_amd as lvk
    from livevisionkit_amd import _native
    names = ("lvk_hip_draw_points", "lvk_hip_draw_rect", "lvk_hip_draw_text", "lvk_hip_text_size")
    lib = _native.load()
    text = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    for name in names:
        assert name in _native.symbols() and hasattr(lib, name)
        assert name + "(" in stable and name + "(" not in experimental
    assert int(re.search(r"#define LVK_HIP_ABI_VERSION (\d+)", text).group(1)) >= 11 and lib.lvk_hip_abi_version() >= 11
    for name in ("draw_points", "draw_rect", "draw_text", "text_size"):
        assert callable(getattr(lvk, name)) and name in lvk.__all__
