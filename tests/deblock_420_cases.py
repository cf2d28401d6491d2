"""Shared by the tests of lvk_hip_deblock_apply_yuv420 (tests/test_deblock_420_spec.py, tests/test_deblock_420_gpu.py, tests/test_deblock_420_facade.py):
the cases, their input planes and -- computed once per case -- the specification's output planes,
    oracle.ingest_yuv420 -> tests/np_deblock.deblock(.., FMT_YUV, ..) -> oracle.egress_yuv420,
the composition tests/test_deblock_facade.py uses for the OBS path."""
import functools

import numpy as np

from tests import np_deblock as nd
from tests.deblock_px_cases import blocky

CASES = [
    # rows, cols, levels, block, k, scaling
    (2, 2, 1, 2, 3, 2.0),               # the smallest frame: every chroma tap is an edge replicate, one block
    (16, 16, 3, 16, 3, 4.0),            # one block; cols = 16 is the dword ingest's lower bound
    (22, 22, 3, 2, 3, 4.0),             # 2 x 2 rule in statistics and downscale; partial cells; cols % 4 != 0
    (30, 34, 4, 3, 3, 2.0),             # region 33 x 30: odd width, quads straddle the right edge
    (34, 30, 4, 3, 3, 2.0),             # region 30 x 33: odd height, quads straddle the bottom edge
    (50, 38, 3, 5, 3, 2.0),             # region 35 x 50: odd width and bs = 5
    (66, 130, 3, 16, 5, 3.0),           # region 128 x 64: area tables; chroma rows and columns wholly outside the region
    (48, 86, 3, 16, 5, 4.0),            # region 80 x 48: ex = 5; ragged row end
    (34, 50, 2, 8, 7, 2.5),             # region 48 x 32: run-time-k median; tables
    (70, 100, 5, 32, 9, 2.5),           # region 96 x 64: 1024-pixel blocks
    (130, 258, 3, 16, 5, 4.0),          # region 256 x 128: more than one thread group per row; a last group of 2 pixels
    (1080, 1920, 3, 16, 5, 4.0),        # region 1920 x 1072: the one full-size case; 8 unfiltered rows
]
NOT_LIVE = [(2, 2), (16, 16)]           # one block, one keep level: the deblocking changes nothing there


def case_id(case):
    return "%dx%d-L%d-b%d-k%d-s%g" % case


def settings(case):
    return dict(detection_levels=case[2], block_size=case[3], filter_size=case[4], filter_scaling=case[5])


def oracle():
    from tests import oracle_lib
    return oracle_lib.load()


def interleave(u, v):
    return np.ascontiguousarray(np.stack([u, v], axis=-1))


def specification(planes, levels, bs, k, s):
    """(output planes (y, u, v), info, ingested packed frame) of I420 planes through the three steps of the definition."""
    o = oracle()
    packed = o.ingest_yuv420(*planes)
    want, info = nd.deblock(packed, nd.FMT_YUV, levels, bs, k, s)
    return o.egress_yuv420(want), info, packed


@functools.lru_cache(maxsize=None)
def expected(case):
    """dict of one case: `planes` (the I420 input), `packed` (its ingest), `want` (the specification's output planes), `info` (np_deblock's) and `trip`
    (the plain ingest -> egress round trip of the input).  Shared between tests, never written to."""
    rows, cols, levels, bs, k, s = case
    o = oracle()
    planes = o.egress_yuv420(blocky(rows, cols, seed=rows * 7 + cols + 3, block=max(bs, 2)))
    want, info, packed = specification(planes, levels, bs, k, s)
    trip = o.egress_yuv420(packed)
    for a in (*planes, *want, *trip, packed):
        a.setflags(write=False)
    return dict(planes=planes, packed=packed, want=want, info=info, trip=trip)


def as_nv12(planes):
    y, u, v = planes
    return y, interleave(u, v)
