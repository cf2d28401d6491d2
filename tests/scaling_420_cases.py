"""Shared by the tests of lvk_hip_scale_yuv420 (tests/test_scaling_420_spec.py, tests/test_scaling_420_gpu.py, tests/test_scaling_420_facade.py): the
cases, their input planes and -- computed once per case and texture -- the specification's output planes,
    oracle.ingest_yuv420 -> oracle.upscale(yuv=True) -> oracle.sharpen -> oracle.egress_yuv420,
with the device reciprocal table as tests/oracle_lib.py sets it up."""
import functools

import numpy as np

SEED = 7
TEXTURES = ["random", "smooth"]

CASES = [
    # source rows, cols, destination rows, cols, sharpness
    (2, 2, 2, 2, 0.8),                  # all border: equals the ingest -> egress round trip
    (2, 2, 4, 4, 0.8),                  # a 2 x 2 interior
    (4, 6, 6, 10, 0.8),
    (8, 8, 8, 8, 0.8),                  # planar route
    (6, 8, 12, 16, 0.8),
    (10, 18, 14, 34, 0.8),              # non-integer factors, cols % 4 == 2, rows % 4 == 2
    (16, 18, 32, 36, 0.8),
    (18, 34, 26, 66, 0.8),
    (34, 66, 70, 130, 0.8),
    (64, 64, 128, 128, 0.8),
    (66, 130, 100, 258, 0.8),           # one column pair past the 256-wide strip
    (130, 254, 196, 508, 0.8),
    (130, 252, 130, 252, 0.8),          # planar route across the strip edge
    (130, 254, 130, 254, 0.8),
    (130, 256, 130, 256, 0.8),
    (130, 260, 130, 260, 0.8),
    (14, 20, 14, 20, 0.8),              # planar route around the block's 16 rows
    (16, 20, 16, 20, 0.8),
    (18, 20, 18, 20, 0.8),
    (270, 480, 540, 960, 0.8),
    (540, 960, 1080, 1920, 0.8),        # the one full-size case
    (18, 34, 26, 66, 0.0),              # the ends of the sharpness range, one per route each
    (18, 34, 26, 66, 1.0),
    (16, 20, 16, 20, 0.0),
    (16, 20, 16, 20, 1.0),
]
C_2x2, C_4x4, C_14x34, C_128, C_258, C_P254 = CASES[0], CASES[1], CASES[5], CASES[9], CASES[10], CASES[13]
# (case at sharpness 0, the same at sharpness 1)
SHARPNESS_ENDS = [(CASES[21], CASES[22]), (CASES[23], CASES[24])]


def case_id(case):
    return "%dx%d-%dx%d-s%g" % case


def equal_sizes(case):
    return case[:2] == case[2:4]


def oracle():
    from tests import oracle_lib
    return oracle_lib.load()


def interleave(u, v):
    return np.ascontiguousarray(np.stack([u, v], axis=-1))


def as_nv12(planes):
    y, u, v = planes
    return y, interleave(u, v)


def layout_of(planes, layout):
    return as_nv12(planes) if layout == "nv12" else tuple(planes)


def texture(kind, rows, cols, seed):
    """I420 planes: `random` = independent bytes; `smooth` = sinusoids plus a few levels of noise."""
    rng = np.random.default_rng(seed)
    planes = []
    for i, (r, c) in enumerate([(rows, cols), (rows // 2, cols // 2), (rows // 2, cols // 2)]):
        if kind == "random":
            planes.append(rng.integers(0, 256, (r, c), dtype=np.uint8))
            continue
        yy, xx = np.mgrid[0:r, 0:c].astype(np.float64) * (1 if i == 0 else 2)
        wave = 128 + 70 * np.sin(xx * (0.21 + 0.05 * i) + 0.3 * i) * np.cos(yy * (0.17 + 0.04 * i)) + 40 * np.sin((xx + yy) * 0.053 + i)
        planes.append(np.clip(np.rint(wave + rng.integers(-3, 4, (r, c))), 0, 255).astype(np.uint8))
    return tuple(planes)


def chain(planes, dst_rows, dst_cols, sharpness, sharpen=True):
    """(output planes (y, u, v), ingested packed frame, upscaled packed frame) of I420 planes through the steps of the definition; sharpen=False leaves
    that step out."""
    o = oracle()
    packed = o.ingest_yuv420(*planes)
    scaled = o.upscale(packed, (dst_cols, dst_rows), yuv=True)
    return o.egress_yuv420(o.sharpen(scaled, sharpness) if sharpen else scaled), packed, scaled


@functools.lru_cache(maxsize=None)
def expected(case, kind="random"):
    """dict of one case and texture: `planes` (the I420 input), `packed` (its ingest), `scaled` (the upscaled packed frame) and `want` (the
    specification's output planes).  Shared between tests, never written to."""
    rows, cols, drows, dcols, sharpness = case
    planes = texture(kind, rows, cols, SEED)
    want, packed, scaled = chain(planes, drows, dcols, sharpness)
    for a in (*planes, *want, packed, scaled):
        a.setflags(write=False)
    return dict(planes=planes, packed=packed, scaled=scaled, want=want)
