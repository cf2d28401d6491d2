"""The tracker's image entries refuse a pitch shorter than its row with LVK_HIP_ERR_ARG, like the remap entries (remap_plane_ok), and write nothing."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG, FILL = -1, 0x5A


def _dev(shape, value=0, dtype=None):
    import torch
    return torch.full(shape, value, dtype=dtype or torch.uint8, device="cuda")


def _untouched(ctx, t):
    ctx.sync()
    return bool((t == (FILL if t.element_size() == 1 else 0x5A5A)).all())


def test_err_arg_is_what_the_header_says():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lvk_hip.h")).read()
    assert int(re.search(r"LVK_HIP_ERR_ARG\s*=?\s*(-?\d+)", text).group(1)) == ERR_ARG


def test_luma_area_resize_refuses_short_pitches(ctx):
    lib, h = ctx.lib, ctx.handle
    src, dst = _dev((16 * 48,)), _dev((8 * 16,), FILL)
    # (src_step, pix_stride, scols) with src_step < scols * pix_stride; then dst_step < dcols; every kind of scale
    for srows, scols, pix, step in ((16, 16, 3, 47), (16, 16, 1, 15), (12, 12, 4, 47), (4, 4, 2, 7)):
        assert lib.lvk_hip_luma_area_resize(h, src.data_ptr(), step, pix, 0, srows, scols, dst.data_ptr(), 8, 8, 8) == ERR_ARG
        assert b"pre-condition" in lib.lvk_hip_last_error(h)
    for srows, scols in ((16, 16), (12, 12), (4, 4)):
        assert lib.lvk_hip_luma_area_resize(h, src.data_ptr(), 48, 3, 0, srows, scols, dst.data_ptr(), 7, 8, 8) == ERR_ARG
    assert _untouched(ctx, dst)
    assert lib.lvk_hip_luma_area_resize(h, src.data_ptr(), 48, 3, 0, 16, 16, dst.data_ptr(), 8, 8, 8) == 0
    ctx.sync()
    assert bool((dst[:64] == 0).all()) and bool((dst[64:] == FILL).all())


def test_pyr_down_refuses_short_pitches(ctx):
    lib, h = ctx.lib, ctx.handle
    src, dst = _dev((9 * 16,)), _dev((5 * 8 + 8,), FILL)
    assert lib.lvk_hip_pyr_down(h, src.data_ptr(), 14, 9, 15, dst.data_ptr(), 8) == ERR_ARG        # src_step < cols
    assert lib.lvk_hip_pyr_down(h, src.data_ptr(), 16, 9, 15, dst.data_ptr(), 7) == ERR_ARG        # dst_step < (cols + 1) / 2
    assert _untouched(ctx, dst)
    assert lib.lvk_hip_pyr_down(h, src.data_ptr(), 16, 9, 15, dst.data_ptr(), 8) == 0
    ctx.sync()
    assert bool((dst[:40] == 0).all()) and bool((dst[40:] == FILL).all())


def test_scharr_refuses_a_short_pitch(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    src, dst = _dev((9 * 16,)), _dev((9 * 15 * 2 + 8,), 0x5A5A, torch.int16)
    assert lib.lvk_hip_scharr(h, src.data_ptr(), 14, 9, 15, dst.data_ptr()) == ERR_ARG
    assert _untouched(ctx, dst)
    assert lib.lvk_hip_scharr(h, src.data_ptr(), 15, 9, 15, dst.data_ptr()) == 0
    ctx.sync()
    assert bool((dst[:270] == 0).all()) and bool((dst[270:] == 0x5A5A).all())


def test_build_pyramid_refuses_a_short_pitch(ctx):
    lib, h = ctx.lib, ctx.handle
    rows, cols = 40, 40
    src = _dev((rows * cols,))
    lv = np.full(rows * cols * 2, FILL, np.uint8); dv = np.full(rows * cols * 4, 0x5A5A, np.int16)
    lr = np.full(8, 0x5A5A5A5A, np.int32); lc = np.full(8, 0x5A5A5A5A, np.int32)
    args = (lv.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), dv.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
            lr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), lc.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert lib.lvk_hip_build_pyramid(h, src.data_ptr(), cols - 1, rows, cols, 3, 11, 11, *args) == ERR_ARG
    assert (lv == FILL).all() and (dv == 0x5A5A).all() and (lr == 0x5A5A5A5A).all() and (lc == 0x5A5A5A5A).all()
    assert lib.lvk_hip_build_pyramid(h, src.data_ptr(), cols, rows, cols, 3, 11, 11, *args) == 2
    assert (lr[:2] == [40, 20]).all()


def test_fast_detect_refuses_a_short_pitch(ctx):
    lib, h = ctx.lib, ctx.handle
    rows, cols = 16, 32
    img = _dev((rows * cols,))
    regions = np.array([0, 0, cols, rows, 10, 1], np.int32)
    out = np.full(64, 0x5A5A5A5A, np.uint32); counts = np.full(1, 0x5A5A5A5A, np.int32)
    args = (regions.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 64,
            counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert lib.lvk_hip_fast_detect(h, img.data_ptr(), cols - 1, rows, cols, *args) == ERR_ARG
    assert (out == 0x5A5A5A5A).all() and counts[0] == 0x5A5A5A5A
    assert lib.lvk_hip_fast_detect(h, img.data_ptr(), cols, rows, cols, *args) == 0
    assert counts[0] == 0
