"""Shared by the tests of lvk_hip_remap_map_yuv420 and the lens filter object (tests/test_lens_420_spec.py, tests/test_lens_420_gpu.py,
tests/test_lc_filter_facade.py): the cases, their inputs and -- computed once per case -- the specification's outputs, from the oracle's
ingest_yuv420, draw_grid, lens_offset_map, remap_map and egress_yuv420, with the device reciprocal table as tests/oracle_lib.py sets it up."""
import functools

import numpy as np

from tests.scaling_420_cases import TEXTURES, as_nv12, interleave, layout_of, oracle, texture   # noqa: F401  (re-exported)
from tests.test_lens_gpu import PROFILES

SEED = 11
BG = (9, 99, 199)                                  # the primitive's background in the tests
MAGENTA_YUV, MAGENTA_BGR = (105, 212, 234), (255, 0, 255)
GRID = (32, 32)

# ---- the primitive: packed YUV frame + offset map -> planes ------------------------------------------------------------------------------------------
# rows x cols: cols % 4 == 2, rows % 4 == 2, both sides of the 256-column and the 4-row strip, the npx == 2 chroma tail, one full-size frame
PRIM_SIZES = [(2, 2), (4, 6), (6, 8), (8, 10), (14, 18), (16, 34), (18, 66), (34, 130), (66, 254), (66, 256), (66, 258), (130, 260), (270, 480), (1080, 1920)]
MAPS = ["near", "far", "lens", "nonfinite"]


def size_id(size):
    return "%dx%d" % tuple(size)


def maps_of(size):
    """The maps a size is run with: the lens map needs a frame the profile's view region is defined on (from 8 x 10 up)."""
    return [m for m in MAPS if m != "lens" or (size[0] >= 8 and size[1] >= 10)]


def offset_map(name, rows, cols):
    rng = np.random.default_rng(rows * 7 + cols + MAPS.index(name))
    if name == "near":
        return rng.uniform(-3, 3, (rows, cols, 2)).astype(np.float32)
    if name == "far":
        return rng.uniform(-1.5 * cols, 1.5 * cols, (rows, cols, 2)).astype(np.float32)        # mostly out of bounds
    if name == "lens":
        return oracle().lens_offset_map(PROFILES[0](rows, cols), rows, cols)[0]
    m = rng.uniform(-2, 2, (rows, cols, 2)).astype(np.float32)                                 # NaN, +-inf and 1e30 entries among small offsets
    bad = [(np.nan, 0), (np.inf, 1), (-np.inf, -np.inf), (1e30, -1e30), (0, np.nan), (-1e30, 1e30)]
    for k in range(max(6, rows * cols // 16)):
        m[rng.integers(rows), rng.integers(cols)] = bad[k % len(bad)]
    return m


@functools.lru_cache(maxsize=None)
def packed_source(rows, cols, kind):
    src = oracle().ingest_yuv420(*texture(kind, rows, cols, SEED))
    src.setflags(write=False)
    return src


def prim_texture(size):
    """1080p runs one texture; every other size both."""
    return ["smooth"] if size[0] >= 1080 else TEXTURES


@functools.lru_cache(maxsize=None)
def prim_expected(size, name, kind):
    """dict: `src` (packed YUV frame), `map` (offsets), `remapped` (the packed destination the chain would write), `want` (I420 planes)."""
    rows, cols = size
    o = oracle()
    src, m = packed_source(rows, cols, kind), offset_map(name, rows, cols)
    remapped = o.remap_map(src, m, bg=BG, yuv=True, nthreads=16)
    want = o.egress_yuv420(remapped)
    for a in (m, remapped, *want):
        a.setflags(write=False)
    return dict(src=src, map=m, remapped=remapped, want=want)


def classify(m, rows, cols):
    """Per output pixel the path remap_one_strip takes: 0 = EASU, 1 = border copy, 2 = background.  (int)coord truncates, saturates and maps NaN to 0."""
    def trunc(v):
        with np.errstate(invalid="ignore"):
            v = np.where(np.isnan(v), np.float32(0), v)
            return np.clip(np.trunc(v.astype(np.float64)), -2**31, 2**31 - 1).astype(np.int64)
    jj, ii = np.meshgrid(np.arange(cols, dtype=np.float32), np.arange(rows, dtype=np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = trunc(jj + m[..., 0]), trunc(ii + m[..., 1])
    easu = (sx >= 1) & (sy >= 1) & (sx < cols - 4) & (sy < rows - 4)
    inside = (sx >= 0) & (sx < cols) & (sy >= 0) & (sy < rows)
    return np.where(easu, 0, np.where(inside, 1, 2))


# ---- the filter: planes -> planes ---------------------------------------------------------------------------------------------------------------------
FILTER_SIZES = [(8, 10), (16, 34), (66, 258), (270, 480)]
SEQUENCE_SIZES = [(66, 130), (34, 66)]
FILTER_PROFILES = [0, 1, 3, None]


def params_of(profile, rows, cols):
    """The nine parameters of profile `profile` (an index into PROFILES, or None) as tests/test_lens_gpu.py scales them to a rows x cols frame."""
    return None if profile is None else tuple(float(v) for v in PROFILES[profile](rows, cols))


def profile_id(p):
    return "none" if p is None else "p%d" % p


@functools.lru_cache(maxsize=None)
def lens_map(profile, rows, cols, at=None):
    """(offset map, view) of a rows x cols frame under the profile scaled to the frame, or -- a camera whose frames change size -- to the size `at`."""
    m, view = oracle().lens_offset_map(params_of(profile, *(at or (rows, cols))), rows, cols)
    m.setflags(write=False)
    return m, view


@functools.lru_cache(maxsize=None)
def filter_expected(size, profile, test_mode, kind, at=None):
    """dict: `planes` (I420 input), `want` (I420 output of ingest -> [grid] -> [remap_map, bg 0] -> egress), `round_trip` (ingest -> egress), `view`.
    at: the frame size the profile's parameters are scaled to (None: this one)."""
    rows, cols = size
    o = oracle()
    planes = texture(kind, rows, cols, SEED)
    packed = packed_source(rows, cols, kind)
    round_trip = o.egress_yuv420(packed)
    if test_mode:
        packed = o.draw_grid(packed, GRID, MAGENTA_YUV, 1)
    view = (0, 0, cols, rows)
    if profile is not None:
        m, view = lens_map(profile, rows, cols, at)
        packed = o.remap_map(packed, m, bg=(0, 0, 0), yuv=True, nthreads=16)
    want = o.egress_yuv420(packed)
    for a in (*planes, *want, *round_trip):
        a.setflags(write=False)
    return dict(planes=planes, want=want, round_trip=round_trip, view=tuple(view))


@functools.lru_cache(maxsize=None)
def packed_expected(size, profile, test_mode, fmt_yuv, kind="smooth"):
    """The packed three-channel apply: dict `src`, `gridded` (the source after the call: with the grid in test mode) and `want`."""
    rows, cols = size
    o = oracle()
    src = packed_source(rows, cols, kind)
    gridded = o.draw_grid(src, GRID, MAGENTA_YUV if fmt_yuv else MAGENTA_BGR, 1) if test_mode else src
    want = gridded if profile is None else o.remap_map(gridded, lens_map(profile, rows, cols)[0], bg=(0, 0, 0), yuv=fmt_yuv)
    for a in (gridded, want):
        a.setflags(write=False)
    return dict(src=src, gridded=gridded, want=want)
