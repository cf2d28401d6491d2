"""The case table of the luma + INTER_AREA downscale (lvk_hip_luma_area_resize): one row per (source size, destination size, pixel stride,
channel, base offset, pitch slack) with the kernel form (LVK_AREA_PATH_* of include/lvk_hip.h) the row is listed under.  Shared by the GPU test
of every form (tests/test_area_resize_paths_gpu.py) and by the CPU check of the oracle against a float64 area mean
(tests/test_area_resize_oracle.py).  The shapes are the smallest that cross the launch geometry: a 5 x 67 destination crosses the 64-column
and the 4-row block boundary and ends ragged on both."""
import collections

import numpy as np

# LVK_AREA_PATH_* (tests/test_area_resize_oracle.py holds this list to the header)
PATHS = {"FAST_DW_8x8_C3_BGR": 0, "FAST_DW_8x8_C3_RGB": 1, "FAST_DW_4x4_C3_BGR": 2, "FAST_DW_4x4_C3_RGB": 3, "FAST_DW_8x8_C3": 4, "FAST_DW_4x4_C3": 5,
         "FAST_DW_8x8_C1": 6, "FAST_DW_4x4_C1": 7, "FAST": 8, "TILE_4": 9, "TILE_8": 10, "TAPS_4": 11, "TAPS_8": 12, "GENERAL": 13, "ENLARGE": 14}
PATH_NAMES = {v: k for k, v in PATHS.items()}

Row = collections.namedtuple("Row", "kind src dst pix ch off slack form twin_of extremes")

DST = (5, 67)
SEED = 4          # of the random content; settled on the CPU so that every row keeps the 2 % cap of tests/test_area_resize_oracle.py
EXACT_SCALES = [(1, 1), (2, 2), (3, 3), (2, 3), (3, 2), (4, 4), (8, 8), (16, 16), (5, 1)]            # (sx, sy)
# the dword-load forms: 4 x 4 and 8 x 8 of packed three-byte pixels (channel 0, BGR -> gray, RGB -> gray) and of a planar source
DWORD_FORMS = {(8, 3, -1): "FAST_DW_8x8_C3_BGR", (8, 3, -2): "FAST_DW_8x8_C3_RGB", (4, 3, -1): "FAST_DW_4x4_C3_BGR", (4, 3, -2): "FAST_DW_4x4_C3_RGB",
               (8, 3, 0): "FAST_DW_8x8_C3", (4, 3, 0): "FAST_DW_4x4_C3", (8, 1, 0): "FAST_DW_8x8_C1", (4, 1, 0): "FAST_DW_4x4_C1"}
# fractional scales s = 68/67, ~69/67, 1.5, 2.67, 3.9, 6.5, 8.5 of the 5 x 67 destination: (source rows, source cols), the largest tap count per
# axis class ("4": <= 4 taps, "8": 5 ... 8, "G": more).  Every width but the literal 68 is no multiple of 4.
FRACTIONAL = [((6, 68), "4"), ((6, 69), "4"), ((7, 101), "4"), ((13, 179), "4"), ((19, 261), "8"), ((33, 435), "8"), ((43, 570), "G")]
ENLARGE = [((180, 320), (270, 480)), ((135, 240), (270, 480)), ((200, 300), (270, 480)), ((400, 300), (270, 480)), ((100, 640), (270, 480)),
           ((269, 479), (270, 480)), ((7, 5), (33, 47)), ((1, 1), DST), ((9, 1), DST), ((1, 9), DST)]


def channels(pix):
    return list(range(pix)) + ([-1, -2] if pix >= 3 else [])


def _table():
    rows = []

    def add(kind, src, dst, pix, ch, off, slack, form, twin_of=None):
        rows.append(Row(kind, src, dst, pix, ch, off, slack, form, twin_of, False))
        return len(rows) - 1

    # ---- exact scales: every stride, every channel ----
    for sx, sy in EXACT_SCALES:
        src = (DST[0] * sy, DST[1] * sx)
        for pix in (1, 2, 3, 4):
            for ch in channels(pix):
                dw = DWORD_FORMS.get((sx, pix, ch)) if sx == sy else None
                if dw:
                    # base and pitch multiples of 4 (67 * 4 * pix is one): the dword form; and its misaligned twins, which fall back
                    aligned = add("exact", src, DST, pix, ch, 0, 0, dw)
                    for off in (1, 2, 3):
                        add("exact", src, DST, pix, ch, off, 0, "FAST", twin_of=aligned)
                    for slack in (1, 2, 3):
                        add("exact", src, DST, pix, ch, 0, slack, "FAST", twin_of=aligned)
                else:
                    add("exact", src, DST, pix, ch, (sx + pix) % 4, (sy + ch) % 4, "FAST")
    # the other destination shapes: one pixel, exactly one block, one row ending one column into the second block
    for dst in ((1, 1), (4, 64), (1, 65)):
        add("exact", (dst[0] * 2, dst[1] * 2), dst, 1, 0, 1, 2, "FAST")
        add("exact", (dst[0] * 4, dst[1] * 4), dst, 3, -1, 0, 0, "FAST_DW_4x4_C3_BGR")
        add("exact", (dst[0] * 8, dst[1] * 8), dst, 1, 0, 0, 0, "FAST_DW_8x8_C1")
        add("exact", (dst[0] * 2, dst[1] * 3), dst, 4, 2, 3, 1, "FAST")
    add("exact", (3, 5), (1, 1), 3, -2, 2, 3, "FAST")

    # ---- fractional scales ----
    tile = {"4": "TILE_4", "8": "TILE_8", "G": "GENERAL"}
    taps = {"4": "TAPS_4", "8": "TAPS_8", "G": "GENERAL"}
    for src, cls in FRACTIONAL:
        pad4 = (-src[1]) % 4                                      # a pitch of whole dwords: the tile kernel's dword loads
        add("frac", src, DST, 1, 0, 0, pad4, tile[cls])
        add("frac", src, DST, 1, 0, 1, 3, tile[cls])              # ... and its byte branch for every load
        add("frac", src, DST, 3, 0, 0, 0, taps[cls])
        add("frac", src, DST, 3, 1, 2, 1, taps[cls])
        add("frac", src, DST, 2, 1, 1, 2, taps[cls])
        add("frac", src, DST, 4, 3, 3, 0, taps[cls])
        add("frac", src, DST, 3, -1, 0, 0, "GENERAL")
        add("frac", src, DST, 4, -2, 1, 1, "GENERAL")
    add("frac", (6, 97), (4, 64), 1, 0, 0, 3, "TILE_4")
    add("frac", (6, 97), (4, 64), 1, 0, 1, 3, "TILE_4")
    add("frac", (3, 253), (1, 65), 3, 1, 0, 1, "TAPS_8")         # exact in y, fractional in x
    add("frac", (3, 253), (1, 65), 1, 0, 0, 3, "TILE_8")
    add("frac", (7, 67), (5, 67), 1, 0, 2, 0, "TILE_4")          # fractional in y only

    # ---- towards a larger image on either axis ----
    for src, dst in ENLARGE:
        add("enlarge", src, dst, 2, 1, 1, 3, "ENLARGE")
        add("enlarge", src, dst, 4, -1, 2, 1, "ENLARGE")
        add("enlarge", src, dst, 4, -2, 3, 2, "ENLARGE")
        add("enlarge", src, dst, 4, 2, 0, 0, "ENLARGE")

    # the saturating ends of the rounding (all-0, all-255, checkerboard): the first exact and the first fractional row of every form
    seen = set()
    for i, r in enumerate(rows):
        if (r.form, r.kind) not in seen:
            seen.add((r.form, r.kind))
            rows[i] = r._replace(extremes=True)
    return rows


TABLE = _table()


def row_id(i):
    r = TABLE[i]
    return "%d-%s-%dx%d-to-%dx%d-p%dc%d-o%ds%d" % (i, r.form, r.src[0], r.src[1], r.dst[0], r.dst[1], r.pix, r.ch, r.off, r.slack)


def content(row, kind="random"):
    """The source pixels of a row, [rows, cols, pix] uint8 (pix == 1: [rows, cols]).  Random content depends on the source geometry alone, so
    that a misaligned twin reads what its aligned row reads."""
    srows, scols = row.src
    shape = (srows, scols, row.pix)
    if kind == "random":
        a = np.random.default_rng([srows, scols, row.pix, SEED]).integers(0, 256, shape, dtype=np.uint8)
    elif kind == "zeros":
        a = np.zeros(shape, np.uint8)
    elif kind == "ones":
        a = np.full(shape, 255, np.uint8)
    elif kind == "checker":
        y, x = np.mgrid[0:srows, 0:scols]
        a = np.repeat((((y + x) & 1) * 255).astype(np.uint8)[:, :, None], row.pix, axis=2)
    else:
        raise ValueError(kind)
    return a[:, :, 0] if row.pix == 1 else a
