"""FAST-9/16 + non-max suppression (k_fast_detect: 64 x 8 output tiles with a 4-pixel apron; k_fast_compact: row-major list) where image size
and placement can go wrong: corners on tile seams, on the first and last admissible row and column, images smaller than one tile, regions off
the tile grid, pitched planes.  Against the oracle and, for isolated bright pixels, against the answer written out here."""
import itertools

import numpy as np
import pytest

from tests import synth

gpu = pytest.mark.gpu          # (the checks of the tables themselves need none)

# An isolated 255 on black is a FAST-9 corner at every threshold below 255 (its whole ring is darker by 255; score 254), and nothing else in the
# image is one (a ring that holds the dot has ONE brighter pixel).  Per image size (rows, cols): images as (dots, the dots that must be
# reported, row-major).  A dot whose ring leaves the image -- column 2, row 2, column cols - 3, row rows - 3 and beyond -- must not be.
# Dots of one image lie at least 8 apart.  (x, y) throughout.
DOT_IMAGES = {
    (7, 7): [([(3, 3)], [(3, 3)])],
    (8, 71): [([(3, 3), (67, 4), (35, 2)], [(3, 3), (67, 4)]),
              ([(2, 4), (30, 4), (68, 3)], [(30, 4)]),
              ([(63, 4), (20, 7)], [(63, 4)]),
              ([(64, 3), (20, 5)], [(64, 3)])],
    (16, 64): [([(3, 3), (60, 12), (30, 7), (45, 2), (2, 12)], [(3, 3), (30, 7), (60, 12)]),
               ([(30, 8), (61, 3), (10, 13)], [(30, 8)])],
    (17, 65): [([(3, 3), (61, 13), (30, 7), (45, 2), (2, 13)], [(3, 3), (30, 7), (61, 13)]),
               ([(30, 8), (62, 3), (50, 14)], [(30, 8)]),
               ([(63, 7), (20, 8)], [(20, 8)]),
               ([(64, 8), (40, 7)], [(40, 7)])],
    (9, 129): [([(3, 3), (125, 5), (63, 4), (80, 2), (100, 6)], [(3, 3), (63, 4), (125, 5)]),
               ([(2, 4), (64, 3), (126, 4)], [(64, 3)]),
               ([(63, 3), (127, 4)], [(63, 3)]),
               ([(64, 5), (128, 3)], [(64, 5)])],
    (24, 200): [([(3, 3), (196, 20), (63, 7), (127, 15), (100, 2), (2, 15), (197, 10)], [(3, 3), (63, 7), (127, 15), (196, 20)]),
                ([(64, 8), (128, 16), (20, 21)], [(64, 8), (128, 16)]),
                ([(63, 8), (127, 16), (128, 7)], [(128, 7), (63, 8), (127, 16)]),
                ([(64, 7), (128, 15)], [(64, 7), (128, 15)])],
}
SEAMS_X, SEAMS_Y = (63, 64, 127, 128), (7, 8, 15, 16)


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_dot_images_are_what_they_claim():
    for (rows, cols), images in DOT_IMAGES.items():
        for dots, expect in images:
            assert all(0 <= x < cols and 0 <= y < rows for x, y in dots)
            assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 8 for a, b in itertools.combinations(dots, 2)), (rows, cols, dots)
            assert expect and expect == sorted((d for d in dots if 3 <= d[0] < cols - 3 and 3 <= d[1] < rows - 3), key=lambda d: (d[1], d[0]))
        if (rows, cols) in ((17, 65), (9, 129), (24, 200)):
            assert any(x in SEAMS_X or y in SEAMS_Y for _, expect in images for x, y in expect)
    everything = [d for images in DOT_IMAGES.values() for dots, _ in images for d in dots]
    assert {(3, 3), (63, 7), (64, 8), (63, 8), (64, 7), (127, 15), (128, 16)} <= set(everything)
    for (rows, cols), images in DOT_IMAGES.items():
        assert any((cols - 4, rows - 4) in expect for _, expect in images)
        if cols >= 16:
            unreported = [d for dots, expect in images for d in dots if d not in expect]
            assert any(x == 2 for x, _ in unreported) and any(y == 2 for _, y in unreported) and any(x == cols - 3 for x, _ in unreported)


@gpu
@pytest.mark.parametrize("threshold", [1, 20, 254])
@pytest.mark.parametrize("size", sorted(DOT_IMAGES), ids=lambda s: "%dx%d" % s)
def test_isolated_dots_on_seams_and_edges(ctx, oracle, size, threshold):
    rows, cols = size
    for dots, expect in DOT_IMAGES[size]:
        img = np.zeros(size, np.uint8)
        for x, y in dots:
            img[y, x] = 255
        want = oracle.fast(img, threshold)
        got, counts = ctx.fast_detect(_gpu(img), [(0, 0, cols, rows, threshold, 1)])
        assert counts[0] == len(want) == len(expect), (dots, counts[0], len(want))
        assert np.array_equal(got[0], want), dots
        assert [tuple(k) for k in got[0][:, :2]] == expect, dots
        assert np.array_equal(got[0][:, 2], want[:, 2]) and (got[0][:, 2] == 254).all()


# region lists (x, y, w, h) per textured image size (rows, cols)
REGION_LISTS = {
    (24, 200): [[(0, 0, 200, 24)],                                             # the whole image
                [(5, 3, 131, 19), (70, 9, 65, 15)],                            # origins off the tile grid in x and y
                [(0, 0, 100, 24), (100, 0, 100, 24)],                          # two regions that share an edge
                [(61, 5, 139, 19)],                                            # right and bottom edges are the image's
                [(10, 0, 90, 24), (100, 0, 6, 24), (106, 0, 94, 24)],          # 6 wide: no key point, neighbours unchanged
                [(0, 0, 200, 12), (0, 12, 200, 6), (0, 18, 200, 6)]],          # 6 high
    (41, 131): [[(0, 0, 131, 41)],
                [(3, 5, 120, 30), (65, 9, 66, 17)],
                [(0, 0, 131, 20), (0, 20, 131, 21)],
                [(67, 17, 64, 24)],
                [(0, 0, 60, 41), (60, 0, 6, 41), (66, 0, 65, 41)],
                [(0, 0, 131, 17), (0, 17, 131, 6), (0, 23, 131, 18)]],
}
TEXTURED_SEED = 17


@pytest.fixture(scope="module")
def textured():
    return {size: synth.textured_frame(size[0], size[1], seed=TEXTURED_SEED, channels=1) for size in REGION_LISTS}


def test_textured_region_lists_hold_enough_corners(oracle, textured):
    """By the oracle alone: the lists of each image together hold at least 50 corners at threshold 10, a 6-wide or 6-high region holds none; and
    the dot images' written-out answers are the oracle's."""
    for size, lists in REGION_LISTS.items():
        total = 0
        for regions in lists:
            for roi in regions:
                assert roi[0] >= 0 and roi[1] >= 0 and roi[0] + roi[2] <= size[1] and roi[1] + roi[3] <= size[0]
                n = len(oracle.fast(textured[size], 10, roi=roi))
                assert n == 0 or (roi[2] > 6 and roi[3] > 6)
                total += n
        print(size, "corners at threshold 10 over the region lists:", total)
        assert total >= 50, (size, total)
    for size, images in DOT_IMAGES.items():
        for dots, expect in images:
            img = np.zeros(size, np.uint8)
            for x, y in dots:
                img[y, x] = 255
            assert [tuple(k) for k in oracle.fast(img, 20)] == [(x, y, 254) for x, y in expect]


def _check_regions(ctx, oracle, img, dev, regions, threshold):
    got, counts = ctx.fast_detect(dev, [(x, y, w, h, threshold, 1) for x, y, w, h in regions])
    total = 0
    for i, roi in enumerate(regions):
        want = oracle.fast(img, threshold, roi=roi)
        assert counts[i] == len(want), (regions, i, counts[i], len(want))
        assert np.array_equal(got[i], want), (regions, i)
        if roi[2] == 6 or roi[3] == 6:
            assert len(want) == 0
        total += len(want)
    return total


@gpu
@pytest.mark.parametrize("threshold", [1, 10, 254])
@pytest.mark.parametrize("size", sorted(REGION_LISTS), ids=lambda s: "%dx%d" % s)
def test_textured_region_placements(ctx, oracle, textured, size, threshold):
    img = textured[size]
    dev = _gpu(img)
    total = sum(_check_regions(ctx, oracle, img, dev, regions, threshold) for regions in REGION_LISTS[size])
    if threshold == 10:
        assert total >= 50, total


@gpu
def test_textured_pitched_source(ctx, oracle, textured):
    import torch
    img = textured[(24, 200)]
    rows, cols = img.shape
    pitch = cols + 5
    host = np.full(64 + 1 + rows * pitch + 64, 0xEE, np.uint8)
    host[65:65 + rows * pitch].reshape(rows, pitch)[:, :cols] = img
    buf = torch.from_numpy(host).cuda()
    view = torch.as_strided(buf, (rows, cols), (pitch, 1), 65)
    total = sum(_check_regions(ctx, oracle, img, view, regions, 10) for regions in REGION_LISTS[(24, 200)])
    assert total >= 50
    assert np.array_equal(buf.cpu().numpy(), host)


@gpu
def test_capacity_truncates_inside_the_first_tile_row(ctx, oracle, textured):
    img = textured[(24, 200)]
    want = oracle.fast(img, 10)
    cap = 3
    assert len(want) > cap and want[cap, 1] < 8, "the cut must fall inside the first tile row"
    got, counts = ctx.fast_detect(_gpu(img), [(0, 0, 200, 24, 10, 1)], cap=cap)
    assert counts[0] == len(want)
    assert np.array_equal(got[0], want[:cap])
