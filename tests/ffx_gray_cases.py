"""Shared by the tests of CAS and FSR EASU on one-channel frames (tests/test_ffx_gray_spec.py, tests/test_ffx_gray_gpu.py): the definitions
(DESIGN.md section 24), evaluated with the THREE-channel specifications tests/np_cas.py and tests/np_fsr.py, the cases the device runs, and
-- computed once per case -- what the definitions make of them.

  CAS, GRAY   channel 0 of np_cas.cas((g, g, g), sharpness)
  EASU, GRAY  channel 0 of np_fsr.fsr((g, g, g), fmt, region, out_rows, out_cols) for any three-channel fmt"""
import functools

import numpy as np

from tests import np_cas as nc
from tests import np_fsr as nf
from tests.test_cas_gpu import content

BGR, RGB, YUV = nf.FMT_BGR, nf.FMT_RGB, nf.FMT_YUV
SHARPNESS = [0.0, 0.25, 0.37, 0.8, 1.0]
LIVE = 0.25                                 # the share of a case's bytes that the filter must change
LIVE_PIXELS = 16                            # ... for cases of this many pixels or more (frame, and for EASU region and output)


def grey3(g):
    return np.repeat(g[..., None], 3, axis=2)


def cas_gray(g, sharpness):
    return nc.cas(grey3(g), sharpness)[..., 0]


def fsr_gray(g, region, out_rows, out_cols, fmt=BGR):
    return nf.fsr(grey3(g), fmt, region, out_rows, out_cols)[..., 0]


def nearest(g, region, out_rows, out_cols):
    """The nearest texel of the region for every output pixel: what a scaler that does no filtering would emit."""
    rx, ry, rw, rh = region
    ys = ry + np.minimum((np.arange(out_rows) * 2 + 1) * rh // (2 * out_rows), rh - 1)
    xs = rx + np.minimum((np.arange(out_cols) * 2 + 1) * rw // (2 * out_cols), rw - 1)
    return g[np.ix_(ys, xs)]


def frame(rows, cols, seed):
    """tests/test_cas_gpu.py's content with one channel: random bytes with a flat patch and a ramp, so that every branch of the clamps is taken."""
    return content(rows, cols, 1, seed)[..., 0]


def centred(rows, cols, seed):
    """`frame` rolled by a quarter of its size: the flat patch in the middle, so that a crop at any corner of the frame holds texture."""
    return np.roll(frame(rows, cols, seed), (rows // 4, cols // 4), axis=(0, 1))


def sweep(transposed):
    """Every byte value in every neighbour position against centres of every value: (x + 7 y) mod 256 on 258 x 258, and its transpose."""
    y, x = np.mgrid[0:258, 0:258]
    return ((y + 7 * x if transposed else x + 7 * y) % 256).astype(np.uint8)


# ---- CAS.  k_cas_gray: a thread owns 4 pixels (one dword) of 4 rows, a wave a strip of 256 pixels, a block 16 rows, and a misaligned destination
# row shifts the groups by up to 3 pixels: one below, at and above each of these widths and heights, besides the sizes of tests/test_cas_gpu.py.
CAS_SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (7, 1), (3, 5), (17, 31), (16, 64), (17, 65),
             (5, 3), (5, 4), (5, 5), (5, 8), (3, 9), (4, 9), (15, 9), (33, 9),
             (5, 252), (5, 253), (5, 255), (5, 256), (5, 257), (4, 259), (3, 515)]
PADS = [(1, 13), (13, 64), (64, 1), (0, 13)]                 # (source, destination) pitch padding: odd pitches
OFFSETS = [(1, 2), (3, 0), (0, 3), (2, 1)]                   # (source, destination) byte offset of the frame in its buffer
CAS_PAD_SIZES = [(37, 131), (5, 70), (2, 3)]
CAS_FLAT = [255, 254, 128, 200]                              # 20 x 70 frames of one value
CAS_SWEEP_SHARPNESS = [0.0, 0.8, 1.0]
# Not held to LIVE: the flat frames and the two sweeps.  Their second differences vanish (everywhere, and everywhere but at the wrap of the
# sweep), so they are fixed points of a sharpener by construction: the definition changes 7 to 8 % of a sweep's bytes.  The flat frames are about
# the error of the approximate reciprocals where it changes a byte (255 -> 254, 254 -> 253, the border of 200 -> 199), the sweeps about every byte
# value meeting every neighbour position; both are compared bit for bit like every other case.
CAS_REF = (270, 480, 0.8)                                    # against the compiled reference shader text


def cas_frame(case):
    """The input of a CAS case: ("size", rows, cols, k) | ("pad", rows, cols) | ("sweep", transposed) | ("flat", value) | ("ref",)."""
    kind = case[0]
    if kind == "size":
        return frame(case[1], case[2], seed=case[1] * 100 + case[2] + case[3])
    if kind == "pad":
        return frame(case[1], case[2], seed=case[1] + case[2])
    if kind == "sweep":
        return sweep(case[1])
    if kind == "flat":
        return np.full((20, 70), case[1], np.uint8)
    assert kind == "ref"
    return frame(CAS_REF[0], CAS_REF[1], seed=270)


def cas_live_cases():
    """(case, sharpness) of every CAS run of the GPU test that LIVE applies to."""
    out = [(("size", r, c, k), s) for r, c in CAS_SIZES for k, s in enumerate(SHARPNESS)]
    out += [(("pad", r, c), 0.8) for r, c in CAS_PAD_SIZES]
    out += [(("ref",), CAS_REF[2])]
    return out


@functools.lru_cache(maxsize=None)
def cas_expected(case, sharpness):
    """(input, the definition's output) of one CAS case; shared between tests, never written to."""
    g = cas_frame(case)
    want = cas_gray(g, sharpness)
    for a in (g, want):
        a.setflags(write=False)
    return g, want


# ---- EASU.  The lists of tests/test_fsr_gpu.py.
SMALL_IN = [(1, 1), (1, 2), (2, 1), (3, 5), (16, 64), (17, 65)]
SMALL_OUT = [(1, 1), (1, 7), (5, 1), (2, 3), (7, 11), (16, 64), (33, 130), (65, 17)]
# (the crops run on `centred`: `frame` is flat in its upper left quarter, where the first crop lies)
CROPS = [(0, 0, 20, 15), (37, 0, 20, 15), (0, 25, 20, 15), (37, 25, 20, 15), (1, 1, 55, 38), (56, 39, 1, 1), (0, 0, 57, 1)]       # on 40 x 57
STAGED_3 = [((0, 0, 500, 300), 700, 1100), ((3, 5, 400, 250), 250, 400), ((0, 0, 500, 300), 1, 1)]                             # on 300 x 500
DIRECT_3 = [((0, 0, 500, 300), 150, 250), ((0, 0, 500, 300), 30, 400), ((7, 2, 480, 290), 290, 100), ((0, 0, 500, 300), 200, 333),
            ((0, 0, 500, 300), 5, 7)]
FSR_PAD_SIZES = [(37, 131, 50, 201), (5, 70, 3, 35), (2, 3, 4, 5)]
FSR_ALIGN = [(33, 63), (33, 64), (33, 65)]                   # 17 x 65 to one column below, at and above the 64-pixel tile, at every alignment
FSR_REF = [((0, 0, 480, 270), 540, 960), ((120, 67, 240, 135), 270, 480)]                                                       # on 270 x 480


def fsr_cases():
    """(rows, cols, seed, region, out_rows, out_cols, centred) of every distinct EASU run of the GPU test; LIVE applies to all of them."""
    out = [(r, c, r * 100 + c, (0, 0, c, r), oh, ow, False) for r, c in SMALL_IN for oh, ow in SMALL_OUT]
    out += [(40, 57, sum(reg), reg, oh, ow, True) for reg in CROPS for oh, ow in ((reg[3] * 2, reg[2] * 2), (31, 17), (1, 1))]
    out += [(300, 500, oh, reg, oh, ow, False) for reg, oh, ow in STAGED_3 + DIRECT_3]
    out += [(r, c, r + c, (0, 0, c, r), oh, ow, False) for r, c, oh, ow in FSR_PAD_SIZES]
    out += [(17, 65, 1765, (0, 0, 65, 17), oh, ow, False) for oh, ow in FSR_ALIGN]
    out += [(270, 480, 270, reg, oh, ow, False) for reg, oh, ow in FSR_REF]
    return out


@functools.lru_cache(maxsize=None)
def fsr_expected(rows, cols, seed, region, out_rows, out_cols, in_the_middle=False):
    """(input, the definition's output) of one EASU case; shared between tests, never written to."""
    g = (centred if in_the_middle else frame)(rows, cols, seed)
    want = fsr_gray(g, region, out_rows, out_cols)
    for a in (g, want):
        a.setflags(write=False)
    return g, want
