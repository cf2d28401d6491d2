"""Shared by the one- and four-channel deblocking tests (tests/test_deblock_px_spec.py, tests/test_deblock_px_gpu.py) and by the three-channel tests
that run the same small and edge cases (tests/test_deblock_spec.py, tests/test_deblock_gpu.py): the cases, their input textures and -- computed once
per case -- what the specification (tests/np_deblock_px.py, tests/np_deblock.py) makes of them."""
import functools

import numpy as np

from tests import np_deblock as nd
from tests import np_deblock_px as npx

GRAY, BGRA, RGBA = npx.FMT_GRAY, npx.FMT_BGRA, npx.FMT_RGBA
VARIANTS = [GRAY, BGRA, RGBA]
NAMES = {GRAY: "gray", BGRA: "bgra", RGBA: "rgba"}

CASES = [
    # rows, cols, levels, block, k, scaling, pad (GRAY: bytes; three and four channels: pixels)
    (67, 131, 3, 16, 5, 3.0, 3),        # area tables (1 / (double)(1.f / 3) != 3), register median 5, region 128 x 64 inside the frame
    (131, 67, 1, 2, 3, 2.0, 5),         # 2 x 2 (sum + 2) >> 2 both in stats and downscale, one level
    (64, 96, 3, 16, 5, 4.0, 4),         # integer box rule 4 x 4; aligned rows
    (64, 96, 3, 16, 5, 2.0, 8),
    (48, 85, 3, 16, 5, 4.0, 2),         # ex = 5: a part-filled group of four waves; ragged row end
    (31, 29, 4, 3, 3, 2.0, 1),          # 9-pixel blocks (fewer than a wave), small size rounded up -> partial cells
    (22, 22, 3, 2, 3, 4.0, 7),          # small 6 x 6 from 22: cells past the region
    (33, 50, 2, 8, 7, 2.5, 3),          # run-time-k LDS median, tables
    (70, 100, 5, 32, 9, 2.5, 6),        # 1024-pixel blocks, 16 values per lane
    (40, 37, 3, 8, 115, 2.0, 9),        # median beyond kMedLdsMaxK (global reads), window larger than the image
    (16, 16, 3, 16, 3, 4.0, 1),         # one block, 4 x 4 small image
    (720, 1280, 5, 8, 7, 3.0, 12),      # the one large case: many tiles and strips
]
NOT_LIVE = (16, 16)                     # one block: one keep level; the liveness condition does not apply


def case_id(case):
    return "%dx%d-L%d-b%d-k%d-s%g" % case[:6]


def blocky(rows, cols, seed, block=16, channels=3):
    """tests/test_deblock_gpu.py's compressed-looking frame with the channel count as a parameter: flat block x block tiles with noise of a per-tile
    amplitude (0-12) and a few fully textured tiles, so that several keep levels occur.  [rows, cols] for channels == 1; alpha is textured like a
    colour channel."""
    rng = np.random.default_rng(seed)
    th, tw = (rows + block - 1) // block, (cols + block - 1) // block

    def up(a):
        return np.repeat(np.repeat(a, block, axis=0), block, axis=1)[:rows, :cols]

    base, amp = up(rng.integers(0, 256, (th, tw, channels))), up(rng.integers(0, 13, (th, tw, 1)))
    f = base + np.rint((rng.random((rows, cols, channels)) * 2 - 1) * amp).astype(np.int64)
    tex = up(rng.random((th, tw)) < 0.1)
    f = np.where(tex[..., None], rng.integers(0, 256, (rows, cols, channels)), f)
    f = np.clip(f, 0, 255).astype(np.uint8)
    return f[..., 0] if channels == 1 else f


def channels_of(fmt):
    return 1 if fmt == GRAY else 4


@functools.lru_cache(maxsize=None)
def expected(case, fmt):
    """(input, specification's output, info) of one case and pixel format; shared between tests, never written to."""
    rows, cols, levels, bs, k, s, _ = case
    c = channels_of(fmt)
    img = blocky(rows, cols, seed=rows * 7 + cols + c, block=max(bs, 2), channels=c)
    want, info = npx.deblock_px(img, fmt, levels, bs, k, s)
    for a in (img, want):
        a.setflags(write=False)
    return img, want, info


@functools.lru_cache(maxsize=None)
def expected3(case, fmt):
    """(input, specification's output, info) of one case as a three-channel frame of format BGR / RGB / YUV; shared between tests, never written to."""
    rows, cols, levels, bs, k, s, _ = case
    img = blocky(rows, cols, seed=rows * 7 + cols + 3, block=max(bs, 2), channels=3)
    want, info = nd.deblock(img, fmt, levels, bs, k, s)
    for a in (img, want):
        a.setflags(write=False)
    return img, want, info
