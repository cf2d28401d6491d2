"""Shared by the tests of lvk_hip_remap_map_obs and lvk_hip_lens_apply_obs (tests/test_lens_obs_spec.py, tests/test_lens_obs_gpu.py,
tests/test_lens_obs_facade.py): the cases, their inputs and -- computed once per case -- the specification's outputs, from the oracle's ingest_obs,
draw_grid, lens_offset_map, remap_map and egress_obs.  Maps, profiles, textures, BG and classify are those of tests/lens_420_cases.py."""
import functools

import numpy as np

from tests.lens_420_cases import (BG, GRID, MAGENTA_BGR, MAGENTA_YUV, TEXTURES, classify, lens_map, maps_of, offset_map, oracle, packed_source,  # noqa: F401
                                  params_of, profile_id, size_id)

GUARD = 0x5A                                       # what the output planes hold before a call: bytes the egress leaves alone keep it

FORMATS = ["I420", "NV12", "YVYU", "YUY2", "UYVY", "RGBA", "BGRA", "BGRX", "Y800", "I444", "BGR3", "I422", "I40A", "I42A", "YUVA", "AYUV"]
F420 = ["I420", "I40A", "NV12"]
F422 = ["I422", "I42A", "YUY2", "YVYU", "UYVY"]
F444 = ["I444", "YUVA", "AYUV"]
FUSABLE = F422 + F444                              # lvk_remap_obs_fusable
DIRECT4 = ["RGBA", "BGRA", "BGRX"]
FRAME_YUV = F420 + FUSABLE                         # lvk_hip_obs_frame_format == LVK_FORMAT_YUV


def plane_shapes(fmt, rows, cols):
    return oracle().obs_plane_shapes(fmt, rows, cols)


@functools.lru_cache(maxsize=None)
def packed_texture(rows, cols, kind):
    """A packed [rows, cols, 3] frame of any size: the packed source of tests/lens_420_cases.py at the next even size, cut to rows x cols."""
    src = np.ascontiguousarray(packed_source(rows + (rows & 1), cols + (cols & 1), kind)[:rows, :cols])
    src.setflags(write=False)
    return src


def guard_planes(fmt, rows, cols):
    return [np.full(sh, GUARD, np.uint8) for sh in plane_shapes(fmt, rows, cols)]


def egress(fmt, frame):
    """oracle.egress_obs into planes that hold GUARD: what the call leaves of an output buffer pre-filled with it."""
    rows, cols = frame.shape[:2]
    return oracle().egress_obs(fmt, frame, guard_planes(fmt, rows, cols))


@functools.lru_cache(maxsize=None)
def input_planes(fmt, rows, cols, kind):
    src = packed_texture(rows, cols, kind)
    planes = egress(fmt, src[..., 0] if fmt == "Y800" else src)
    for p in planes:
        p.setflags(write=False)
    return tuple(planes)


# ---- the primitive: packed YUV frame + offset map -> planes of a fusable format --------------------------------------------------------------------------
# odd rows; cols % 4 == 2, the sinks' npx == 2 tail; both sides of the 256-column and the 4-row strip
PRIM_SIZES_444 = [(2, 2), (3, 5), (5, 7), (8, 10), (9, 13), (17, 35), (19, 67), (66, 254), (66, 255), (66, 256), (66, 257), (67, 258), (131, 261), (270, 480)]
PRIM_SIZES_422 = [(2, 2), (3, 6), (5, 10), (8, 10), (9, 18), (17, 34), (19, 66), (66, 254), (66, 256), (66, 258), (67, 260), (270, 480)]
PRIM_FULL = [("UYVY", (1080, 1920)), ("I444", (1080, 1920))]            # `smooth` only


def prim_sizes(fmt):
    return PRIM_SIZES_422 if fmt in F422 else PRIM_SIZES_444


PRIM_CASES = [(f, s) for f in FUSABLE for s in prim_sizes(f)] + PRIM_FULL


def case_id(case):
    return "%s-%s" % (case[0], size_id(case[1]))


def prim_textures(size):
    return ["smooth"] if size[0] >= 1080 else TEXTURES


@functools.lru_cache(maxsize=None)
def prim_remapped(size, name, kind):
    """(src, map, remapped): the packed YUV source, the offsets and the packed frame lvk_hip_remap_map(yuv = 1, BG) writes -- shared by the formats."""
    rows, cols = size
    src, m = packed_texture(rows, cols, kind), offset_map(name, rows, cols)
    remapped = oracle().remap_map(src, m, bg=BG, yuv=True, nthreads=16)
    for a in (m, remapped):
        a.setflags(write=False)
    return src, m, remapped


@functools.lru_cache(maxsize=None)
def prim_expected(fmt, size, name, kind):
    """dict: `src`, `map`, `remapped` and `want` (the planes of `fmt`, GUARD where the egress writes nothing)."""
    src, m, remapped = prim_remapped(size, name, kind)
    want = egress(fmt, remapped)
    for a in want:
        a.setflags(write=False)
    return dict(src=src, map=m, remapped=remapped, want=tuple(want))


# ---- the filter: planes -> planes ---------------------------------------------------------------------------------------------------------------------
FILTER_SIZES = [(8, 10), (16, 34), (66, 258), (270, 480)]
FILTER_SIZES_ODD = [(9, 13), (67, 258)]                                   # formats without 4:2:0 subsampling; 4:2:2 takes the even width next to 13
FILTER_PROFILES = [0, 1, 3, None]


def filter_sizes(fmt):
    if fmt in F420:
        return list(FILTER_SIZES)
    return FILTER_SIZES + [(r, c + (c & 1)) if fmt in F422 else (r, c) for r, c in FILTER_SIZES_ODD]


def chain(fmt, planes, profile, test_mode, at=None):
    """The definition on the oracle: ingest_obs -> [draw_grid] -> [remap_map, bg 0] -> egress_obs into GUARD planes.  Returns (planes, view)."""
    o = oracle()
    frame = o.ingest_obs(fmt, planes)
    rows, cols = frame.shape[:2]
    yuv = fmt in FRAME_YUV
    if test_mode:
        assert fmt != "Y800", "the grid kernel writes three bytes per pixel: refused"
        frame = o.draw_grid(frame, GRID, MAGENTA_YUV if yuv else MAGENTA_BGR, 1)
    view = (0, 0, cols, rows)
    if profile is not None:
        m, view = lens_map(profile, rows, cols, at)
        if fmt == "Y800":                          # channel 0 of the non-YUV program on (g, c, c): lvk_hip_remap_map_gray, DESIGN.md section 19
            frame = np.ascontiguousarray(o.remap_map(np.stack([frame, frame, frame], axis=2), m, bg=(0, 0, 0), yuv=False, nthreads=16)[..., 0])
        else:
            frame = o.remap_map(frame, m, bg=(0, 0, 0), yuv=yuv, nthreads=16)
    return egress(fmt, frame), tuple(view)


@functools.lru_cache(maxsize=None)
def filter_expected(fmt, size, profile, test_mode, kind, at=None):
    """dict: `planes` (the input), `want` (the output planes, GUARD where nothing is written), `round_trip` (ingest -> egress), `view`."""
    rows, cols = size
    planes = input_planes(fmt, rows, cols, kind)
    want, view = chain(fmt, planes, profile, test_mode, at)
    round_trip, _ = chain(fmt, planes, None, False)
    for a in (*want, *round_trip):
        a.setflags(write=False)
    return dict(planes=planes, want=tuple(want), round_trip=tuple(round_trip), view=view)


def filter_cases():
    """(fmt, size, profile, test mode) of every filter case that runs; Y800 in test mode is a refusal and is tested as one."""
    return [(f, s, p, t) for f in FORMATS for s in filter_sizes(f) for p in FILTER_PROFILES for t in (False, True) if not (t and f == "Y800")]


def written_mask(fmt, rows, cols):
    """Per output plane: True where lvk_hip_egress_obs writes.  Everything, except the last quarter of data[0] of the 4-byte DirectIngest formats."""
    masks = [np.ones(sh, bool) for sh in plane_shapes(fmt, rows, cols)]
    if fmt in DIRECT4:
        flat = masks[0].reshape(-1)
        flat[rows * cols * 3:] = False
    return masks
