"""CPU check of the oracle's luma + INTER_AREA downscale at every pixel stride and channel of the case table (tests/area_resize_cases.py)
against something independent of it: the area-weighted mean in plain numpy float64."""
import os
import re

import numpy as np
import pytest

from tests import area_resize_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_case_table_names_the_enum_of_the_header():
    text = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bLVK_AREA_PATH_(\w+) = (\d+)", text)}
    count = enum.pop("COUNT")
    assert enum == cases.PATHS and sorted(enum.values()) == list(range(count))


def test_case_table_reaches_every_form_and_twins_every_dword_row():
    assert {r.form for r in cases.TABLE} == set(cases.PATHS)
    for i, r in enumerate(cases.TABLE):
        if r.form.startswith("FAST_DW") and r.dst == cases.DST:
            twins = [(t.off, t.slack) for t in cases.TABLE if t.twin_of == i]
            assert sorted(twins) == [(0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)], i
            assert all(t.form == "FAST" and (t.src, t.dst, t.pix, t.ch) == (r.src, r.dst, r.pix, r.ch) for t in cases.TABLE if t.twin_of == i)
    # the saturating contents run on an exact row of every integer-scale form and on a fractional row of every fractional-scale form
    marked = {(r.form, r.kind) for r in cases.TABLE if r.extremes}
    assert marked == {(r.form, r.kind) for r in cases.TABLE}


def gray_of(frame, ch):
    """The selected channel, or the 15-bit fixed-point grey of BGR (-1) / RGB (-2): integer and exact."""
    f = frame.astype(np.int64)
    if f.ndim == 2:
        return f
    if ch >= 0:
        return f[:, :, ch]
    b, g, r = (f[:, :, 0], f[:, :, 1], f[:, :, 2]) if ch == -1 else (f[:, :, 2], f[:, :, 1], f[:, :, 0])
    return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15


def area_weights(ssize, dsize):
    """W[d, s] = the share of destination cell d = [d * scale, (d + 1) * scale) that source pixel s covers; and the largest number of
    source pixels a cell touches."""
    scale = ssize / dsize
    w = np.zeros((dsize, ssize), np.float64)
    for d in range(dsize):
        lo, hi = d * scale, min((d + 1) * scale, float(ssize))
        for s in range(int(np.floor(lo)), min(int(np.ceil(hi)), ssize)):
            w[d, s] = max(0.0, min(hi, s + 1.0) - max(lo, float(s))) / scale
    return w, int((w > 0).sum(axis=1).max())


def _unique_rows():
    seen, out = set(), []
    for i, r in enumerate(cases.TABLE):
        key = (r.src, r.dst, r.pix, r.ch)
        if r.kind != "enlarge" and key not in seen:
            seen.add(key)
            out.append(i)
    return out


@pytest.mark.parametrize("i", _unique_rows(), ids=cases.row_id)
def test_oracle_equals_the_float64_area_mean(oracle, i):
    """Bar: the oracle equals the float64 area-weighted mean, rounded half to even, at every pixel whose float64 value lies further from an
    x.5 tie than the margin -- twice the binary32 accumulation bound of the row, (taps_x + taps_y + 2) * 255 * 2^-24; within the margin
    |difference| <= 1, and at most 2 % of a row's pixels may lie there.

    An exact scale with an even box area puts a fixed share of its pixels ON a tie (sum mod area == area / 2: a quarter of them at 2 x 2,
    a sixth at 2 x 3, 1 / 16 at 4 x 4), whatever the seed.  Those are not excused: the integer sum decides them exactly, and they are held to
    equality with OpenCV's rule -- half to even, and half UP, (s + 2) >> 2, in the dedicated 2 x 2 kernel.  The margin then holds only what
    is near a tie without being one.  Largest share inside the margin over the table: 1.49 % (5 of 335 pixels, the
    6 x 68 source at stride 3, channel 1, whose weights are multiples of 1 / 408; the exact rows: none)."""
    r = cases.TABLE[i]
    frame = cases.content(r)
    got = oracle.luma_area_resize(frame, r.dst[0], r.dst[1], channel=r.ch).astype(np.int64)
    g = gray_of(frame, r.ch)
    wy, ty = area_weights(r.src[0], r.dst[0])
    wx, tx = area_weights(r.src[1], r.dst[1])
    val = wy @ g.astype(np.float64) @ wx.T
    margin = 2.0 * (tx + ty + 2) * 255.0 * 2.0 ** -24
    want = np.rint(val).astype(np.int64)
    near = np.abs(val - np.floor(val) - 0.5) <= margin
    equal = np.ones_like(near)
    if r.kind == "exact":
        sx, sy = r.src[1] // r.dst[1], r.src[0] // r.dst[0]
        assert (tx, ty) == (sx, sy)
        s = g.reshape(r.dst[0], sy, r.dst[1], sx).sum(axis=(1, 3))
        tie = 2 * (s % (sx * sy)) == sx * sy
        q = s // (sx * sy)
        decided = (s + 2) >> 2 if (sx, sy) == (2, 2) else q + (q & 1)
        assert np.array_equal(got[tie], decided[tie])
        near &= ~tie
        equal = ~tie                                              # (decided above)
    share = near.mean()
    print("row %s: taps %d x %d, margin %.3g, inside the margin %d of %d pixels (%.2f %%)" % (cases.row_id(i), tx, ty, margin, near.sum(), near.size, 100 * share))
    equal &= ~near
    assert np.array_equal(got[equal], want[equal])
    assert np.abs(got - want)[near].max(initial=0) <= 1
    assert share <= 0.02


def test_fractional_rows_run_from_two_to_ten_taps():
    taps = set()
    for r in cases.TABLE:
        if r.kind == "frac":
            taps.add(max(area_weights(r.src[1], r.dst[1])[1], area_weights(r.src[0], r.dst[0])[1]))
    assert min(taps) == 2 and max(taps) == 10 and {2, 3, 4, 5, 8, 10} <= taps, taps
