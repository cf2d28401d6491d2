"""Shared by the tests of lvk_hip_deblock_apply_obs (tests/test_deblock_obs_spec.py, tests/test_deblock_obs_gpu.py, tests/test_deblock_obs_facade.py): the
cases, their input planes and -- computed once per case -- the specification's output planes,
    oracle.ingest_obs -> tests/np_deblock.deblock(.., FMT_YUV / FMT_BGR / FMT_RGB, ..) -> oracle.egress_obs into planes that hold GUARD,
for Y800 the one-channel definition of tests/np_deblock_px.py between the ingest and the egress.  The texture is tests/deblock_px_cases.blocky, egressed
to the format; GUARD, egress and written_mask are those of tests/lens_obs_cases.py; the 4:2:0 formats take the planes and the cases of
tests/deblock_420_cases.py, whose route they share."""
import functools

import numpy as np

from tests import deblock_420_cases as c420
from tests import np_deblock as nd
from tests import np_deblock_px as npx
from tests.deblock_px_cases import blocky
from tests.lens_obs_cases import DIRECT4, F420, F422, F444, FORMATS, FRAME_YUV, FUSABLE, GUARD, egress, oracle, plane_shapes, written_mask  # noqa: F401

# rows, cols, levels, block, k, scaling
CASES_EVEN = [
    (2, 2, 1, 2, 3, 2.0),               # every chroma tap is an edge replicate, one block: not live
    (3, 6, 2, 2, 3, 2.0),               # odd rows: the last row pair holds one row
    (9, 14, 3, 2, 3, 4.0),              # cols % 4 == 2: a last group of two columns; partial cells
    (17, 34, 4, 3, 3, 2.0),             # region 33 x 15: a 4:2:2 pair straddles the right edge
    (35, 38, 3, 5, 3, 2.0),             # bs = 5, odd region
    (66, 130, 3, 16, 5, 3.0),           # area tables; rows and columns wholly outside the region
    (48, 86, 3, 16, 5, 4.0),            # the defaults; ragged row end
    (34, 50, 2, 8, 7, 2.5),             # run-time-k median; tables
    (66, 254, 3, 16, 5, 4.0),           # either side of the 256-column strip of a 64-thread row
    (67, 258, 3, 16, 5, 4.0),
]
CASES_ODD = [                           # formats that take odd widths: 4:4:4 planar, AYUV, BGR3, the 4-byte formats, Y800
    (3, 5, 2, 2, 3, 2.0),
    (9, 13, 3, 2, 3, 4.0),
    (17, 35, 4, 3, 3, 2.0),
    (67, 257, 3, 16, 5, 4.0),
]
CASES_420 = [c for c in c420.CASES if c[0] < 1080]     # the route is lvk_hip_deblock_apply_yuv420's, so the cases are too
FULL = (1080, 1920, 3, 16, 5, 4.0)                     # on UYVY and I444 only
NOT_LIVE = [(2, 2)] + list(c420.NOT_LIVE)              # one block, one keep level: the deblocking changes nothing there


def cases_of(fmt):
    return CASES_420 if fmt in F420 else CASES_EVEN if fmt in F422 else CASES_EVEN + CASES_ODD


# (format, case)
CASES = [(f, c) for f in FORMATS for c in cases_of(f)]
FULL_CASES = [(f, FULL) for f in ("UYVY", "I444")]
ALL_CASES = CASES + FULL_CASES


def case_id(fc):
    return "%s-%dx%d-L%d-b%d-k%d-s%g" % (fc[0], *fc[1])


def settings(case):
    return dict(detection_levels=case[2], block_size=case[3], filter_size=case[4], filter_scaling=case[5])


def frame_format(fmt):
    """lvk_hip_obs_frame_format: what the ingested frame is"""
    return npx.FMT_GRAY if fmt == "Y800" else nd.FMT_YUV if fmt in FRAME_YUV else nd.FMT_RGB if fmt == "RGBA" else nd.FMT_BGR


@functools.lru_cache(maxsize=None)
def inputs(fmt, case):
    """The planes of one frame of `fmt`: for 4:2:0 the I420 planes of tests/deblock_420_cases.py (interleaved for NV12), else the blocky texture of the
    case egressed to the format (Y800: its channel 0)."""
    rows, cols, levels, bs, k, s = case
    if fmt in F420:
        planes = c420.expected(case)["planes"]
        planes = c420.as_nv12(planes) if fmt == "NV12" else planes
    else:
        tex = blocky(rows, cols, seed=rows * 7 + cols + 3, block=max(bs, 2))
        planes = egress(fmt, np.ascontiguousarray(tex[..., 0]) if fmt == "Y800" else tex)
    for p in planes:
        p.setflags(write=False)
    return tuple(planes)


def chain(fmt, planes, case, deblock=True):
    """(output planes with GUARD where the egress writes nothing, info, ingested frame) through the steps of the definition; deblock=False: the plain
    ingest -> egress round trip."""
    rows, cols, levels, bs, k, s = case
    frame = oracle().ingest_obs(fmt, list(planes))
    info = None
    out = frame
    if deblock:
        if fmt == "Y800":
            out, info = npx.deblock_px(frame, npx.FMT_GRAY, levels, bs, k, s)
        else:
            out, info = nd.deblock(frame, frame_format(fmt), levels, bs, k, s)
    return egress(fmt, out), info, frame


@functools.lru_cache(maxsize=None)
def expected(fmt, case):
    """dict of one format and case: `planes` (the input), `packed` (its ingest), `want` (the specification's output planes, GUARD where nothing is
    written), `info` (np_deblock's) and `trip` (the plain ingest -> egress round trip).  Shared between tests, never written to."""
    planes = inputs(fmt, case)
    want, info, packed = chain(fmt, planes, case)
    trip, _, _ = chain(fmt, planes, case, deblock=False)
    for a in (*want, *trip, packed):
        a.setflags(write=False)
    return dict(planes=planes, packed=packed, want=tuple(want), info=info, trip=tuple(trip))


def live(case):
    return tuple(case[:2]) not in NOT_LIVE


def changed_share(fmt, case):
    """The share of the bytes the egress writes that the deblocking changes: want against the plain round trip."""
    e = expected(fmt, case)
    masks = written_mask(fmt, *case[:2])
    differ = sum(int((w[m] != t[m]).sum()) for w, t, m in zip(e["want"], e["trip"], masks))
    return differ / sum(int(m.sum()) for m in masks)
