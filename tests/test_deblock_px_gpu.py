"""lvk::DeblockingFilter on GRAY and BGRA / RGBA frames on the MI355X (lvk_hip_deblock_apply_gray / _c4), bit for bit against the numpy
restatement (tests/np_deblock_px.py).  Every frame is a view of a wider buffer of random guard bytes: what lies outside the region -- the rest of the
frame, the row padding, the bytes before and behind the frame -- must come back unchanged."""
import ctypes

import numpy as np
import pytest

from tests import np_deblock as nd
from tests import np_deblock_px as npx
from tests.deblock_px_cases import BGRA, CASES, GRAY, NAMES, RGBA, VARIANTS, blocky, case_id, channels_of, expected

pytestmark = pytest.mark.gpu

ERR_ARG = -1


def device_frame(img, pad_bytes=0, offset=0, guard_seed=0):
    """img ([rows, cols] or [rows, cols, 4]) on the GPU as a view, `offset` bytes into a buffer of random guard bytes, with a row pitch of
    BPP * cols + pad_bytes.  Returns (whole buffer on the GPU, the view, the buffer's bytes on the host)."""
    import torch
    rows, cols = img.shape[:2]
    bpp = 1 if img.ndim == 2 else 4
    pitch = bpp * cols + pad_bytes
    flat = np.random.default_rng(guard_seed).integers(0, 256, offset + rows * pitch + 16, dtype=np.uint8)
    host_view(flat, img.shape, pitch, offset)[...] = img
    t = torch.from_numpy(flat).cuda()
    strides = (pitch, 1) if bpp == 1 else (pitch, 4, 1)
    return t, t.as_strided(tuple(img.shape), strides, offset), flat


def host_view(flat, shape, pitch, offset):
    strides = (pitch, 1) if len(shape) == 2 else (pitch, 4, 1)
    return np.lib.stride_tricks.as_strided(flat[offset:], shape=shape, strides=strides)


def expect(flat, want, pad_bytes=0, offset=0):
    out = flat.copy()
    bpp = 1 if want.ndim == 2 else 4
    host_view(out, want.shape, bpp * want.shape[1] + pad_bytes, offset)[...] = want
    return out


def settings(levels, bs, k, s):
    return dict(detection_levels=levels, block_size=bs, filter_size=k, filter_scaling=s)


def tap_equals(f, info):
    mean, grid, keep = f.grid()
    return np.array_equal(mean, info["mean"]) and np.array_equal(grid, info["grid"]) and np.array_equal(keep, info["keep_block"])


@pytest.mark.parametrize("fmt", VARIANTS, ids=[NAMES[v] for v in VARIANTS])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_apply_bit_exact(ctx, case, fmt):
    import livevisionkit_amd as lvk
    img, want, info = expected(case, fmt)
    pad = case[6] * (1 if fmt == GRAY else 4)
    buf, view, flat = device_frame(img, pad, guard_seed=case[4])
    f = lvk.DeblockingFilter(ctx, **settings(*case[2:6]))
    region = f.apply(view, fmt)
    ctx.sync()
    assert region == info["region"] == f.filter_region()
    got, want_buf = buf.cpu().numpy(), expect(flat, want, pad)
    assert np.array_equal(got, want_buf), "%d bytes differ" % int((got != want_buf).sum())
    assert tap_equals(f, info)
    f.close()


@pytest.mark.parametrize("fmt,offset,pad", [(BGRA, 4, 4), (RGBA, 8, 12), (GRAY, 1, 2), (GRAY, 2, 4), (GRAY, 3, 0), (GRAY, 0, 1)])
def test_base_offsets_and_odd_pitches(ctx, fmt, offset, pad):
    # c4: a base 4 and 8 bytes above the allocation; GRAY: bases 1 to 3 bytes above a dword boundary with an odd pitch (131 + even), so that the rows of
    # one frame start at every misalignment, and an aligned base with a pitch that is a multiple of 4 (131 + 1)
    import livevisionkit_amd as lvk
    case = CASES[0]
    img, want, info = expected(case, fmt)
    buf, view, flat = device_frame(img, pad, offset, guard_seed=offset)
    assert view.data_ptr() % 4 == offset % 4
    f = lvk.DeblockingFilter(ctx, **settings(*case[2:6]))
    assert f.apply(view, fmt) == info["region"]
    ctx.sync()
    assert np.array_equal(buf.cpu().numpy(), expect(flat, want, pad, offset))
    f.close()


def raw_apply(f, fmt, ptr, step, rows, cols, cfmt=None):
    if fmt == GRAY:
        return f.lib.lvk_hip_deblock_apply_gray(f.handle, ptr, step, rows, cols, None)
    return f.lib.lvk_hip_deblock_apply_c4(f.handle, ptr, step, rows, cols, fmt if cfmt is None else cfmt, None)


@pytest.mark.parametrize("fmt", VARIANTS, ids=[NAMES[v] for v in VARIANTS])
def test_refused_calls_change_nothing(ctx, fmt):
    import livevisionkit_amd as lvk
    c = channels_of(fmt)
    case = CASES[2]                                              # 64 x 96, the defaults
    img, want, info = expected(case, fmt)
    pad = 4
    buf, view, flat = device_frame(img, pad)
    rows, cols, step, ptr = img.shape[0], img.shape[1], view.stride(0), view.data_ptr()

    fresh = lvk.DeblockingFilter(ctx)
    assert raw_apply(fresh, fmt, None, step, rows, cols) == ERR_ARG
    assert fresh.filter_region() == (0, 0, 0, 0)
    with pytest.raises(lvk.LvkHipError):
        fresh.grid()                                             # still nothing applied
    with pytest.raises(lvk.LvkHipError):
        fresh.draw_influence(device_frame3(64, 96)[1], nd.FMT_YUV)
    fresh.close()

    f = lvk.DeblockingFilter(ctx)
    f.apply(view, fmt)
    ctx.sync()
    applied = buf.cpu().numpy()
    assert np.array_equal(applied, expect(flat, want, pad))

    def unchanged():
        ctx.sync()
        return np.array_equal(buf.cpu().numpy(), applied) and f.filter_region() == info["region"] and tap_equals(f, info)

    refused = [(None, step, rows, cols), (ptr, step, 0, cols), (ptr, step, -3, cols), (ptr, step, rows, 0), (ptr, step, rows, -1),
               (ptr, c * cols - 1, rows, cols)]
    if fmt != GRAY:
        refused += [(ptr + 2, step, rows, cols - 1), (ptr + 1, step, rows, cols - 1), (ptr, step + 2, rows, cols)]    # base / pitch no multiple of 4
    for args in refused:
        assert raw_apply(f, fmt, *args) == ERR_ARG, args
        assert unchanged(), args
    if fmt != GRAY:
        for bad in (0, 2, 4, 5, 6, -1):                          # BGR, RGB, YUV, GRAY, unknown
            assert raw_apply(f, fmt, ptr, step, rows, cols, cfmt=bad) == ERR_ARG, bad
            with pytest.raises(lvk.LvkHipError):
                f.apply(view, bad)
            assert unchanged(), bad

    low = blocky(15, 200, seed=6, channels=c)                    # no whole 16 x 16 block
    lbuf, lview, lflat = device_frame(low, pad)
    with pytest.raises(lvk.LvkHipError):
        f.apply(lview, fmt)
    assert unchanged()
    f.configure(filter_size=257)                                 # accepted by configure, refused by apply
    with pytest.raises(lvk.LvkHipError):
        f.apply(view, fmt)
    assert unchanged()
    f.configure(block_size=2, filter_scaling=8.0)
    tiny = blocky(2, 2, seed=7, channels=c)
    tbuf, tview, tflat = device_frame(tiny)
    with pytest.raises(lvk.LvkHipError):
        f.apply(tview, fmt)                                      # rint(2 / 8) = 0: empty downscale
    ctx.sync()
    assert np.array_equal(lbuf.cpu().numpy(), lflat) and np.array_equal(tbuf.cpu().numpy(), tflat)
    assert np.array_equal(buf.cpu().numpy(), applied) and f.filter_region() == info["region"]
    f.configure()
    assert tap_equals(f, info)
    f.close()


def device_frame3(rows, cols, seed=0):
    import torch
    img = blocky(rows, cols, seed=seed, channels=3)
    return img, torch.from_numpy(img).cuda()


def test_a_three_channel_tensor_of_a_four_channel_format_is_still_refused(ctx):
    import livevisionkit_amd as lvk
    f = lvk.DeblockingFilter(ctx)
    img, t = device_frame3(64, 96, seed=5)
    for fmt in (BGRA, RGBA, GRAY):
        with pytest.raises(lvk.LvkHipError):
            f.apply(t, fmt)
    ctx.sync()
    assert np.array_equal(t.cpu().numpy(), img) and f.filter_region() == (0, 0, 0, 0)
    f.close()


@pytest.mark.parametrize("fmt", [GRAY, BGRA], ids=[NAMES[GRAY], NAMES[BGRA]])
def test_draw_influence_after_a_px_apply_uses_its_maps(ctx, fmt):
    import livevisionkit_amd as lvk
    case = CASES[0]
    img, want, info = expected(case, fmt)
    _, view, _ = device_frame(img)
    f = lvk.DeblockingFilter(ctx, **settings(*case[2:6]))
    f.apply(view, fmt)
    _, _, RW, RH = info["region"]
    img3, t3 = device_frame3(RH, RW, seed=9)                     # an 8UC3 frame of the region's size
    for fmt3 in (nd.FMT_YUV, nd.FMT_BGR):
        t = t3.clone()
        f.draw_influence(t, fmt3)
        ctx.sync()
        assert np.array_equal(t.cpu().numpy(), nd.draw_influence(img3, fmt3, info))
    f.close()


def test_one_handle_across_pixel_sizes_equals_fresh_filters(ctx):
    import torch
    import livevisionkit_amd as lvk
    shared = lvk.DeblockingFilter(ctx)
    steps = [(GRAY, 67, 131), (nd.FMT_BGR, 48, 85), (BGRA, 64, 96), (GRAY, 48, 85)]
    for i, (fmt, rows, cols) in enumerate(steps):
        c = 3 if fmt == nd.FMT_BGR else channels_of(fmt)
        img = blocky(rows, cols, seed=50 + i, channels=c)
        want, info = nd.deblock(img, fmt) if c == 3 else npx.deblock_px(img, fmt)
        a, b = torch.from_numpy(img).cuda(), torch.from_numpy(img).cuda()
        fresh = lvk.DeblockingFilter(ctx)
        assert shared.apply(a, fmt) == fresh.apply(b, fmt) == info["region"]
        ctx.sync()
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and np.array_equal(a.cpu().numpy(), want), (i, fmt)
        assert tap_equals(shared, info) and shared.filter_region() == fresh.filter_region()
        fresh.close()
    shared.close()
