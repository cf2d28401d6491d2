"""lvk::DeblockingFilter on one-channel (GRAY, [rows, cols]) and four-channel (BGRA / RGBA, [rows, cols, 4]) uint8 frames: the operation order of
tests/np_deblock.py (DESIGN.md section 13's table) per channel, composed from that file's channel-generic steps.

The reference's filter is made of channel-agnostic OpenCV calls (Filters/DeblockingFilter.cpp:48-110), so nothing here is a definition of ours:
  grey   GRAY: the frame itself.  BGRA / RGBA: (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15 of the colour bytes, alpha ignored
         (BGRA2GRAY / RGBA2GRAY; np_convert.reformat(.., GRAY), and np_deblock.gray_of on frame[..., :3]).
  alpha  byte 3 of a four-channel frame is a channel like the others: downscaled, median-filtered, up-sampled and blended with the same keep map.
Everything else -- the region of whole macroblocks, small_size, the area fast path / tables at scale 1 / (double)(1.f / s), the exact median with
BORDER_REPLICATE, the 11-bit 8U bilinear, keep_block, the float bilinear keep, the IEEE-divide blend -- is np_deblock's."""
import numpy as np

from tests import np_deblock as nd

FMT_BGRA, FMT_RGBA, FMT_GRAY = 1, 3, 5      # LVK_FORMAT_* of include/lvk_hip.h


def gray_px(region, fmt):
    """reformatTo(GRAY) of a [h, w] GRAY or [h, w, 4] BGRA / RGBA image, int32."""
    if region.ndim == 2:
        return region.astype(np.int32)
    if fmt not in (FMT_BGRA, FMT_RGBA):
        raise ValueError("a four-channel frame is BGRA or RGBA")
    return nd.gray_of(region[..., :3], nd.FMT_BGR if fmt == FMT_BGRA else nd.FMT_RGB)


def deblock_px(frame, fmt, detection_levels=3, block_size=16, filter_size=5, filter_scaling=4.0):
    """DeblockingFilter::filter on a copy of `frame` ([rows, cols] or [rows, cols, 4] uint8; `fmt` is ignored for [rows, cols]).  Returns (out, info)
    like np_deblock.deblock; raises ValueError where the library refuses the frame."""
    if not (frame.ndim == 2 or (frame.ndim == 3 and frame.shape[2] == 4)):
        raise ValueError("a [rows, cols] or [rows, cols, 4] frame")
    bs, L, k, s = int(block_size), int(detection_levels), int(filter_size), float(filter_scaling)
    f = frame if frame.ndim == 3 else frame[..., None]
    rows, cols = f.shape[:2]
    ey, ex = rows // bs, cols // bs
    RH, RW = ey * bs, ex * bs
    if ey == 0 or ex == 0:
        raise ValueError("no whole macroblock")
    hs, ws = nd.small_size(RH, s), nd.small_size(RW, s)
    if hs <= 0 or ws <= 0:
        raise ValueError("empty downscale")
    region = f[:RH, :RW]
    scale = 1.0 / float(nd.f32(1) / nd.f32(s))
    small = nd.area_resize(region, hs, ws, scale)
    med = nd.median(small, k)
    smooth = nd.resize_linear_u8(med, RH, RW)
    gray = gray_px(frame[:RH, :RW], fmt)
    mean = nd.block_grid(gray, bs)
    dev = np.abs(gray - np.repeat(np.repeat(mean, bs, axis=0), bs, axis=1))
    grid = nd.block_grid(dev, bs)
    kb = nd.keep_block_of(grid, L)
    keep = nd.resize_linear_f32(kb, RH, RW)
    out = f.copy()
    out[:RH, :RW] = nd.blend(region, smooth, keep)

    def px(a):
        return a if frame.ndim == 3 else a[..., 0]

    info = dict(region=(0, 0, RW, RH), small=px(small), median=px(med), smooth=px(smooth), mean=mean.astype(np.uint8), grid=grid.astype(np.uint8),
                keep_block=kb, keep=keep)
    return px(out), info
