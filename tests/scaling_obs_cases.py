"""Shared by the tests of lvk_hip_scale_obs (tests/test_scaling_obs_spec.py, tests/test_scaling_obs_gpu.py, tests/test_scaling_obs_facade.py): the cases,
their input planes and -- computed once per case and texture -- the specification's output planes,
    oracle.ingest_obs -> oracle.upscale(yuv = the frame format is YUV) -> oracle.sharpen -> oracle.egress_obs into planes that hold GUARD,
for Y800 the one-channel definitions of tests/scaling_px_cases.py between the ingest and the egress.  Textures, input planes and GUARD are those of
tests/lens_obs_cases.py; the 4:2:0 formats take the planes and the cases of tests/scaling_420_cases.py, whose route they share."""
import functools

import numpy as np

from tests import scaling_420_cases as c420
from tests import scaling_px_cases as px
from tests.lens_obs_cases import (DIRECT4, F420, F422, F444, FORMATS, FRAME_YUV, FUSABLE, GUARD, TEXTURES, egress, guard_planes, input_planes,  # noqa: F401
                                  oracle, plane_shapes, written_mask)

SHARPNESS = 0.8

# (source (rows, cols), destination (rows, cols)): the all-border frame; odd rows and cols; both sides of the 256-column strip with every cols % 4; around
# the block's 16 rows with every rows % 4; a destination one column pair past the strip; a quarter of the full size
SIZES_444 = [((2, 2), (2, 2)), ((2, 2), (4, 4)), ((3, 5), (3, 5)), ((3, 5), (5, 9)), ((9, 13), (9, 13)), ((9, 13), (14, 21)), ((17, 35), (17, 35)),
             ((66, 254), (66, 254)), ((66, 255), (66, 255)), ((66, 256), (66, 256)), ((66, 257), (66, 257)), ((67, 258), (67, 258)),
             ((14, 20), (14, 20)), ((16, 20), (16, 20)), ((17, 20), (17, 20)), ((66, 130), (100, 258)), ((135, 240), (270, 480))]
# the same with every width made even
SIZES_422 = [((2, 2), (2, 2)), ((2, 2), (4, 4)), ((3, 6), (3, 6)), ((3, 6), (5, 10)), ((9, 14), (9, 14)), ((9, 14), (14, 22)), ((17, 34), (17, 34)),
             ((66, 254), (66, 254)), ((66, 256), (66, 256)), ((66, 258), (66, 258)), ((67, 260), (67, 260)),
             ((14, 20), (14, 20)), ((16, 20), (16, 20)), ((17, 20), (17, 20)), ((66, 130), (100, 258)), ((135, 240), (270, 480))]
# the route is lvk_hip_scale_yuv420's, so the cases are too
SIZES_420 = [(c[:2], c[2:4]) for c in (c420.C_2x2, c420.C_4x4, c420.C_14x34, c420.C_258, c420.C_P254)]
FULL = ((540, 960), (1080, 1920))                          # on UYVY and I444, `smooth` only


def sizes_of(fmt):
    return SIZES_420 if fmt in F420 else SIZES_422 if fmt in F422 else SIZES_444


# (format, source, destination, sharpness)
CASES = [(f, s, d, SHARPNESS) for f in FORMATS for s, d in sizes_of(f)]
ENDS = [(f, s, d, sh) for f, pairs in (("UYVY", SIZES_422), ("I444", SIZES_444), ("BGR3", SIZES_444)) for s, d in (pairs[5], pairs[6]) for sh in (0.0, 1.0)]
FULL_CASES = [(f, *FULL, SHARPNESS) for f in ("UYVY", "I444")]
ALL_CASES = CASES + ENDS + FULL_CASES


def case_id(case):
    return "%s-%dx%d-%dx%d-s%g" % (case[0], *case[1], *case[2], case[3])


def textures_of(case):
    return ["smooth"] if case[1][0] >= 540 else TEXTURES


def equal_sizes(case):
    return case[1] == case[2]


def family(fmt):
    return "420" if fmt in F420 else "422" if fmt in F422 else "444" if fmt in F444 else "direct4" if fmt in DIRECT4 else fmt


@functools.lru_cache(maxsize=None)
def inputs(fmt, size, kind):
    """The planes of one frame of `fmt`: for 4:2:0 the I420 texture of tests/scaling_420_cases.py (interleaved for NV12), else tests/lens_obs_cases.py's."""
    if fmt in F420:
        planes = c420.texture(kind, *size, c420.SEED)
        planes = c420.as_nv12(planes) if fmt == "NV12" else planes
        for p in planes:
            p.setflags(write=False)
        return tuple(planes)
    return input_planes(fmt, *size, kind)


def chain(fmt, planes, dst, sharpness, sharpen=True):
    """(output planes with GUARD where the egress writes nothing, ingested frame, upscaled frame) through the steps of the definition."""
    o = oracle()
    frame = o.ingest_obs(fmt, list(planes))
    size = (dst[1], dst[0])
    if fmt == "Y800":
        scaled = px.upscale_gray(lambda f, s: o.upscale(f, s, yuv=False), frame, size)
        out = px.sharpen_gray(o.sharpen, scaled, sharpness) if sharpen else scaled
    else:
        scaled = o.upscale(frame, size, yuv=fmt in FRAME_YUV)
        out = o.sharpen(scaled, sharpness) if sharpen else scaled
    return egress(fmt, out), frame, scaled


@functools.lru_cache(maxsize=None)
def expected(case, kind="random"):
    """dict of one case and texture: `planes` (the input), `packed` (its ingest), `scaled` (the upscaled frame) and `want` (the specification's output
    planes, GUARD where nothing is written).  Shared between tests, never written to."""
    fmt, src, dst, sharpness = case
    planes = inputs(fmt, src, kind)
    want, packed, scaled = chain(fmt, planes, dst, sharpness)
    for a in (*want, packed, scaled):
        a.setflags(write=False)
    return dict(planes=planes, packed=packed, scaled=scaled, want=tuple(want))


# ---- the 4:2:2 chroma up-sampling in closed form: what PlaneSrc (csrc/scaling_obs.hip) computes -----------------------------------------------------------
def up2x_row(c):
    """One chroma row [.., cols / 2] -> [.., cols]: (other + 3 * nearer + 2) >> 2, the other sample the left neighbour for an even column and the right one
    for an odd column, the edge sample replicated (up2x, csrc/ingest.hip)."""
    c = c.astype(np.int32)
    left = np.concatenate([c[..., :1], c[..., :-1]], axis=-1)
    right = np.concatenate([c[..., 1:], c[..., -1:]], axis=-1)
    out = np.empty(c.shape[:-1] + (2 * c.shape[-1],), np.int32)
    out[..., 0::2] = (left + 3 * c + 2) >> 2
    out[..., 1::2] = (right + 3 * c + 2) >> 2
    return out.astype(np.uint8)


def split_422(fmt, planes):
    """(Y [rows, cols], U, V [rows, cols / 2]) of the planes of a 4:2:2 format"""
    if fmt in ("I422", "I42A"):
        return planes
    p = planes[0].reshape(planes[0].shape[0], -1, 4)                               # one pixel pair per 4 bytes
    y0, c0, y1, c1 = (0, 1, 2, 3) if fmt != "UYVY" else (1, 0, 3, 2)
    y = np.stack([p[..., y0], p[..., y1]], axis=-1).reshape(p.shape[0], -1)
    first, second = p[..., c0], p[..., c1]
    return (y, second, first) if fmt == "YVYU" else (y, first, second)


def ingest_422_twin(fmt, planes):
    y, u, v = split_422(fmt, planes)
    return np.ascontiguousarray(np.stack([y, up2x_row(u), up2x_row(v)], axis=-1))
