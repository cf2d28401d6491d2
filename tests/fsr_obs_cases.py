"""Shared by the tests of lvk_hip_fsr_yuv420 / lvk_hip_fsr_obs (tests/test_fsr_obs_spec.py, tests/test_fsr_obs_gpu.py, tests/test_fsr_obs_facade.py): the
cases (format, source (rows, cols), region (x, y, w, h) or None for the whole frame, output (rows, cols)), their input planes and -- computed once per case
-- the specification's output planes,
    oracle.ingest_obs -> tests/np_fsr.fsr(.., the format's frame format, region, output size) -> oracle.egress_obs into planes that hold GUARD,
for Y800 the one-channel definition tests/ffx_gray_cases.fsr_gray between the ingest and the egress.  GUARD, egress, written_mask and FORMATS are those of
tests/lens_obs_cases.py.  The inputs are seeded uniform noise, egressed to the format: EASU's direction analysis is flat on constants, so a smooth texture
would leave most of the arithmetic unused.

The sizes are the smallest at which the 64 x 16 output tile, the LDS stage, the sinks' groups of four and the choice between the staged and the direct
path can each go wrong: (2, 2), where every tap is clamped; outputs one short of, equal to and one past the tile; several tiles; a staged downscale; a
staged case just under the stage's 2560 texels ((48, 96) -> (34, 66): 2375) and direct cases on one and on several tiles.  PATHS holds the path each case
was chosen for (0 = staged, 1 = direct: lvk_hip_fsr_obs_path, asserted by tests/test_fsr_obs_spec.py): with another budget the sizes must be chosen anew."""
import functools

import numpy as np

from tests import np_fsr as nf
from tests.ffx_gray_cases import fsr_gray
from tests.lens_obs_cases import DIRECT4, F420, F422, F444, FORMATS, FRAME_YUV, GUARD, egress, oracle, plane_shapes, written_mask  # noqa: F401

STAGED, DIRECT = 0, 1
# (source, output, path)
PAIRS_ODD = [((2, 2), (2, 2), STAGED), ((2, 2), (4, 4), STAGED), ((3, 5), (5, 9), STAGED), ((10, 18), (15, 63), STAGED), ((10, 18), (16, 64), STAGED),
             ((10, 18), (17, 65), STAGED), ((24, 40), (34, 62), STAGED), ((24, 40), (18, 30), STAGED), ((48, 96), (34, 66), STAGED),
             ((40, 80), (16, 64), DIRECT), ((40, 80), (17, 65), DIRECT), ((66, 130), (34, 66), DIRECT)]
PAIRS_422 = [((2, 2), (2, 2), STAGED), ((2, 2), (4, 4), STAGED), ((3, 6), (5, 10), STAGED), ((10, 18), (15, 62), STAGED), ((10, 18), (16, 64), STAGED),
             ((10, 18), (17, 66), STAGED), ((24, 40), (34, 62), STAGED), ((24, 40), (18, 30), STAGED), ((48, 96), (34, 66), STAGED),
             ((40, 80), (16, 64), DIRECT), ((40, 80), (17, 66), DIRECT), ((66, 130), (34, 66), DIRECT)]
PAIRS_420 = [((2, 2), (2, 2), STAGED), ((2, 2), (4, 4), STAGED), ((4, 6), (6, 10), STAGED), ((10, 18), (14, 62), STAGED), ((10, 18), (16, 64), STAGED),
             ((10, 18), (18, 66), STAGED), ((24, 40), (34, 62), STAGED), ((24, 40), (18, 30), STAGED), ((48, 96), (34, 66), STAGED),
             ((40, 80), (16, 64), DIRECT), ((40, 80), (18, 66), DIRECT), ((66, 130), (34, 66), DIRECT)]

CROP_FORMATS = ["I420", "NV12", "I422", "UYVY", "I444", "AYUV", "BGR3", "BGRA", "Y800"]
CROP_FRAME, CROP_OUT = (24, 40), (20, 34)
CROP_REGIONS = [(0, 0, 20, 12), (20, 12, 20, 12), (1, 1, 38, 22), (7, 5, 9, 11), (0, 0, 40, 24)]
CROP_DIRECT = ((66, 130), (3, 1, 120, 60), (16, 32))       # the direct path from a region at an odd origin

FULL = ((540, 960), (1080, 1920))
FULL_FORMATS = ["I420", "UYVY"]


def pairs_of(fmt):
    return PAIRS_420 if fmt in F420 else PAIRS_422 if fmt in F422 else PAIRS_ODD


# (format, source, region, output)
SIZE_CASES = [(f, s, None, d) for f in FORMATS for s, d, _ in pairs_of(f)]
CROP_CASES = ([(f, CROP_FRAME, r, CROP_OUT) for f in CROP_FORMATS for r in CROP_REGIONS]
              + [(f, CROP_DIRECT[0], CROP_DIRECT[1], CROP_DIRECT[2]) for f in CROP_FORMATS])
FULL_CASES = [(f, FULL[0], None, FULL[1]) for f in FULL_FORMATS]
CASES = SIZE_CASES + CROP_CASES

PATHS = {(f, s, None, d): p for f in FORMATS for s, d, p in pairs_of(f)}
PATHS.update({c: (DIRECT if c[1] == CROP_DIRECT[0] else STAGED) for c in CROP_CASES})
PATHS.update({c: STAGED for c in FULL_CASES})


def region_of(case):
    _, src, region, _ = case
    return (0, 0, src[1], src[0]) if region is None else tuple(region)


def case_id(case):
    fmt, src, region, dst = case
    return "%s-%dx%d-%s-%dx%d" % (fmt, *src, "whole" if region is None else "r%d.%d.%d.%d" % tuple(region), *dst)


def first_case(fmt, path):
    """The first several-tile case of `fmt` on `path`: (24, 40) -> (34, 62) staged, (66, 130) -> (34, 66) direct."""
    src = (24, 40) if path == STAGED else (66, 130)
    return next(c for c in SIZE_CASES if c[0] == fmt and c[1] == src)


def frame_format(fmt):
    """The np_fsr format of the packed frame the ingest of `fmt` makes (lvk_hip_obs_frame_format)."""
    return nf.FMT_RGB if fmt == "RGBA" else nf.FMT_BGR if fmt in DIRECT4 + ["BGR3"] else nf.FMT_YUV


@functools.lru_cache(maxsize=None)
def noise(rows, cols, seed=0):
    tex = np.random.default_rng(rows * 1009 + cols + 7919 * seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    tex.setflags(write=False)
    return tex


@functools.lru_cache(maxsize=None)
def inputs(fmt, size):
    """The planes of one frame of `fmt`: seeded uniform noise egressed to the format (Y800: its channel 0)."""
    tex = noise(*size)
    planes = egress(fmt, np.ascontiguousarray(tex[..., 0]) if fmt == "Y800" else tex)
    for p in planes:
        p.setflags(write=False)
    return tuple(planes)


def chain(fmt, planes, region, dst):
    """The output planes (GUARD where the egress writes nothing) through the three steps of the definition."""
    frame = oracle().ingest_obs(fmt, list(planes))
    if fmt == "Y800":
        scaled = fsr_gray(frame, region, dst[0], dst[1])
    else:
        scaled = nf.fsr(frame, frame_format(fmt), region, dst[0], dst[1])
    return egress(fmt, np.ascontiguousarray(scaled))


@functools.lru_cache(maxsize=None)
def expected(case):
    """dict of one case: `planes` (the input) and `want` (the specification's output planes, GUARD where nothing is written).  Shared between tests,
    never written to."""
    fmt, src, _, dst = case
    planes = inputs(fmt, src)
    want = chain(fmt, planes, region_of(case), dst)
    for a in want:
        a.setflags(write=False)
    return dict(planes=planes, want=tuple(want))
