"""Shared by the tests of lvk_hip_cas_yuv420 / lvk_hip_cas_obs (tests/test_cas_obs_spec.py, tests/test_cas_obs_gpu.py, tests/test_cas_obs_facade.py): the
cases, their input planes and -- computed once per case -- the specification's output planes,
    oracle.ingest_obs -> tests/np_cas.cas(.., sharpness) -> oracle.egress_obs into planes that hold GUARD,
for Y800 the one-channel definition tests/ffx_gray_cases.cas_gray between the ingest and the egress.  GUARD, egress, written_mask and FORMATS are those of
tests/lens_obs_cases.py.  The inputs are seeded uniform noise, egressed to the format: CAS leaves constants and linear ramps untouched, so the smooth
textures of the sibling case files would prove nothing here.

The sizes are the smallest at which something can break: (2, 2), where every tap is an edge; cols % 4 == 2, a last group of two columns; odd rows and,
where the format takes them, odd widths; both sides of the 256-column strip of a wave and of the row band of a block (8 rows on 4:2:0, 16 elsewhere)."""
import functools

import numpy as np

from tests import np_cas as nc
from tests.ffx_gray_cases import cas_gray
from tests.lens_obs_cases import DIRECT4, F420, F422, F444, FORMATS, FRAME_YUV, GUARD, egress, oracle, plane_shapes, written_mask  # noqa: F401

SIZES_420 = [(2, 2), (4, 6), (6, 10), (8, 14), (18, 34), (66, 254), (66, 256), (68, 258)]
SIZES_422 = [(2, 2), (3, 6), (9, 14), (17, 34), (66, 254), (66, 256), (67, 258)]
SIZES_ODD = [(3, 5), (9, 13), (17, 35), (67, 257)]         # formats that take odd widths: 4:4:4 planar, AYUV, BGR3, the 4-byte formats, Y800
SHARPNESS = [0.0, 0.8, 1.0]
FULL = (1080, 1920)                                        # on I420 and UYVY, at sharpness 0.8
FULL_FORMATS = ["I420", "UYVY"]
FULL_SHARPNESS = 0.8


def sizes_of(fmt):
    return SIZES_420 if fmt in F420 else SIZES_422 if fmt in F422 else SIZES_422 + SIZES_ODD


# (format, size)
CASES = [(f, s) for f in FORMATS for s in sizes_of(f)]
FULL_CASES = [(f, FULL) for f in FULL_FORMATS]


def sharpness_of(size):
    return [FULL_SHARPNESS] if size == FULL else SHARPNESS


def case_id(fc):
    return "%s-%dx%d" % (fc[0], *fc[1])


@functools.lru_cache(maxsize=None)
def noise(rows, cols):
    tex = np.random.default_rng(rows * 1009 + cols).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
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


def chain(fmt, planes, sharpness):
    """The output planes (GUARD where the egress writes nothing) through the steps of the definition; sharpness None: the plain ingest -> egress
    round trip."""
    frame = oracle().ingest_obs(fmt, list(planes))
    if sharpness is not None:
        frame = cas_gray(frame, sharpness) if fmt == "Y800" else nc.cas(frame, sharpness)
    return egress(fmt, np.ascontiguousarray(frame))


@functools.lru_cache(maxsize=None)
def expected(fmt, size, sharpness):
    """dict of one format, size and sharpness: `planes` (the input), `want` (the specification's output planes, GUARD where nothing is written) and
    `trip` (the plain ingest -> egress round trip).  Shared between tests, never written to."""
    planes = inputs(fmt, size)
    want, trip = chain(fmt, planes, sharpness), chain(fmt, planes, None)
    for a in (*want, *trip):
        a.setflags(write=False)
    return dict(planes=planes, want=tuple(want), trip=tuple(trip))


def changed_shares(fmt, size, sharpness):
    """Per output plane, the share of the bytes the egress writes that the filter changes: want against the plain round trip."""
    e = expected(fmt, size, sharpness)
    masks = written_mask(fmt, *size)
    return [float((w[m] != t[m]).mean()) for w, t, m in zip(e["want"], e["trip"], masks)]
