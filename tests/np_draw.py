"""numpy specification of the device drawing calls (csrc/draw.hip): lvk::draw_points, lvk::draw_rect and lvk::draw_text
on a packed 8UC3 frame.  Every function returns a drawn COPY of `img` and raises ValueError for what the library refuses.

  points  Functions/Drawing.tpp:95-141 and the `points` kernel (Functions/OpenCL/Sources/Drawing.cl:43-69): coordinates scaled like
          cv::multiply(.., CV_32S) (binary32 product, round half to even), then a square of half width (point_size + 1) / 2.
  rect    the band of cv::rectangle(Rect) with SQUARE corners (for thickness 1 that is OpenCV's outline; above 1 OpenCV rounds the joins).
  text    this project's own 5 x 7 font in a 6 x 9 cell -- NOT OpenCV's Hershey glyphs.  FONT below is the specification's own copy of the
          table, drawn as text; the library keeps its copy as bit masks (csrc/draw.hip, kFont).  tests/test_draw_suite_gpu.py renders every
          glyph through both.
"""
import numpy as np

GLYPH_W, GLYPH_H = 5, 7              # the drawn part of a cell
CELL_W, CELL_H = 6, 9                # advance; line height: one blank row above the glyph, one below it
MAX_TEXT = 256                       # bytes
MAX_SCALE, MAX_THICKNESS = 32767, 65535

# printable ASCII 0x20 .. 0x7E in order, seven rows each, top row first, '#' = set
FONT = [
    "...../...../...../...../...../...../.....",   # (space)
    "..#../..#../..#../..#../..#../...../..#..",   # !
    ".#.#./.#.#./.#.#./...../...../...../.....",   # "
    ".#.#./.#.#./#####/.#.#./#####/.#.#./.#.#.",   # #
    "..#../.####/#.#../.###./..#.#/####./..#..",   # $
    "##.../##..#/...#./..#../.#.../#..##/...##",   # %
    ".##../#..#./#.#../.#.../#.#.#/#..#./.##.#",   # &
    "..#../..#../..#../...../...../...../.....",   # '
    "..##./.#.../#..../#..../#..../.#.../..##.",   # (
    ".##../...#./....#/....#/....#/...#./.##..",   # )
    "...../..#../#.#.#/.###./#.#.#/..#../.....",   # *
    "...../..#../..#../#####/..#../..#../.....",   # +
    "...../...../...../...../.##../..#../.#...",   # ,
    "...../...../...../#####/...../...../.....",   # -
    "...../...../...../...../...../.##../.##..",   # .
    "...../....#/...#./..#../.#.../#..../.....",   # /
    ".###./#...#/#..##/#.#.#/##..#/#...#/.###.",   # 0
    "..#../.##../..#../..#../..#../..#../.###.",   # 1
    ".###./#...#/....#/...#./..#../.#.../#####",   # 2
    "#####/...#./..#../...#./....#/#...#/.###.",   # 3
    "...#./..##./.#.#./#..#./#####/...#./...#.",   # 4
    "#####/#..../####./....#/....#/#...#/.###.",   # 5
    "..##./.#.../#..../####./#...#/#...#/.###.",   # 6
    "#####/....#/...#./..#../.#.../.#.../.#...",   # 7
    ".###./#...#/#...#/.###./#...#/#...#/.###.",   # 8
    ".###./#...#/#...#/.####/....#/...#./.##..",   # 9
    "...../.##../.##../...../.##../.##../.....",   # :
    "...../.##../.##../...../.##../..#../.#...",   # ;
    "...#./..#../.#.../#..../.#.../..#../...#.",   # <
    "...../...../#####/...../#####/...../.....",   # =
    ".#.../..#../...#./....#/...#./..#../.#...",   # >
    ".###./#...#/....#/...#./..#../...../..#..",   # ?
    ".###./#...#/....#/.##.#/#.#.#/#.#.#/.###.",   # @
    ".###./#...#/#...#/#...#/#####/#...#/#...#",   # A
    "####./#...#/#...#/####./#...#/#...#/####.",   # B
    ".###./#...#/#..../#..../#..../#...#/.###.",   # C
    "###../#..#./#...#/#...#/#...#/#..#./###..",   # D
    "#####/#..../#..../####./#..../#..../#####",   # E
    "#####/#..../#..../####./#..../#..../#....",   # F
    ".###./#...#/#..../#.###/#...#/#...#/.####",   # G
    "#...#/#...#/#...#/#####/#...#/#...#/#...#",   # H
    ".###./..#../..#../..#../..#../..#../.###.",   # I
    "..###/...#./...#./...#./...#./#..#./.##..",   # J
    "#...#/#..#./#.#../##.../#.#../#..#./#...#",   # K
    "#..../#..../#..../#..../#..../#..../#####",   # L
    "#...#/##.##/#.#.#/#.#.#/#...#/#...#/#...#",   # M
    "#...#/#...#/##..#/#.#.#/#..##/#...#/#...#",   # N
    ".###./#...#/#...#/#...#/#...#/#...#/.###.",   # O
    "####./#...#/#...#/####./#..../#..../#....",   # P
    ".###./#...#/#...#/#...#/#.#.#/#..#./.##.#",   # Q
    "####./#...#/#...#/####./#.#../#..#./#...#",   # R
    ".####/#..../#..../.###./....#/....#/####.",   # S
    "#####/..#../..#../..#../..#../..#../..#..",   # T
    "#...#/#...#/#...#/#...#/#...#/#...#/.###.",   # U
    "#...#/#...#/#...#/#...#/#...#/.#.#./..#..",   # V
    "#...#/#...#/#...#/#.#.#/#.#.#/#.#.#/.#.#.",   # W
    "#...#/#...#/.#.#./..#../.#.#./#...#/#...#",   # X
    "#...#/#...#/#...#/.#.#./..#../..#../..#..",   # Y
    "#####/....#/...#./..#../.#.../#..../#####",   # Z
    ".###./.#.../.#.../.#.../.#.../.#.../.###.",   # [
    "...../#..../.#.../..#../...#./....#/.....",   # \
    ".###./...#./...#./...#./...#./...#./.###.",   # ]
    "..#../.#.#./#...#/...../...../...../.....",   # ^
    "...../...../...../...../...../...../#####",   # _
    ".#.../..#../...#./...../...../...../.....",   # `
    "...../...../.###./....#/.####/#...#/.####",   # a
    "#..../#..../#.##./##..#/#...#/#...#/####.",   # b
    "...../...../.###./#..../#..../#...#/.###.",   # c
    "....#/....#/.##.#/#..##/#...#/#...#/.####",   # d
    "...../...../.###./#...#/#####/#..../.###.",   # e
    "..##./.#..#/.#.../###../.#.../.#.../.#...",   # f
    "...../.####/#...#/#...#/.####/....#/.###.",   # g
    "#..../#..../#.##./##..#/#...#/#...#/#...#",   # h
    "..#../...../.##../..#../..#../..#../.###.",   # i
    "...#./...../..##./...#./...#./#..#./.##..",   # j
    "#..../#..../#..#./#.#../##.../#.#../#..#.",   # k
    ".##../..#../..#../..#../..#../..#../.###.",   # l
    "...../...../##.#./#.#.#/#.#.#/#...#/#...#",   # m
    "...../...../#.##./##..#/#...#/#...#/#...#",   # n
    "...../...../.###./#...#/#...#/#...#/.###.",   # o
    "...../####./#...#/#...#/####./#..../#....",   # p
    "...../.####/#...#/#...#/.####/....#/....#",   # q
    "...../...../#.##./##..#/#..../#..../#....",   # r
    "...../...../.###./#..../.###./....#/####.",   # s
    ".#.../.#.../###../.#.../.#.../.#..#/..##.",   # t
    "...../...../#...#/#...#/#...#/#..##/.##.#",   # u
    "...../...../#...#/#...#/#...#/.#.#./..#..",   # v
    "...../...../#...#/#...#/#.#.#/#.#.#/.#.#.",   # w
    "...../...../#...#/.#.#./..#../.#.#./#...#",   # x
    "...../#...#/#...#/#...#/.####/....#/.###.",   # y
    "...../...../#####/...#./..#../.#.../#####",   # z
    "...#./..#../..#../.#.../..#../..#../...#.",   # {
    "..#../..#../..#../..#../..#../..#../..#..",   # |
    ".#.../..#../..#../...#./..#../..#../.#...",   # }
    "...../...../.#.../#.#.#/...#./...../.....",   # ~
]


def glyph(byte):
    """The 7 x 5 boolean bitmap of a byte; bytes outside 0x20 .. 0x7E draw as '?'."""
    rows = FONT[byte - 0x20 if 0x20 <= byte <= 0x7E else ord("?") - 0x20].split("/")
    return np.array([[c == "#" for c in r] for r in rows], dtype=bool)


def text_bytes(text):
    """The bytes of a string as the C entry sees them: UTF-8 for a str; at most MAX_TEXT of them and no NUL."""
    b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    if len(b) > MAX_TEXT or 0 in b:
        raise ValueError("text of at most %d bytes without NUL" % MAX_TEXT)
    return b


def _frame(img):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("a packed 8UC3 frame is required")
    return img.copy()


def scale_points(pts, scaling=(1.0, 1.0)):
    """cv::multiply(points, Scalar(sx, sy), CV_32S) on 32F data: binary32 product, round half to even; NaN -> 0, clamped to +-2^30 (what
    lvk_hip_draw_crosses does with its points)."""
    p = np.asarray(pts, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.stack([p[:, 0] * np.float32(scaling[0]), p[:, 1] * np.float32(scaling[1])], axis=1)
        v = np.where(np.isnan(v), np.float32(0), np.rint(v))
        return np.clip(v, -2.0 ** 30, 2.0 ** 30).astype(np.int64)


def points(img, pts, colour, point_size=10, scaling=(1.0, 1.0)):
    out = _frame(img)
    if point_size < 1 or not (scaling[0] >= 0 and scaling[1] >= 0):
        raise ValueError("point_size >= 1 and scales >= 0")
    rows, cols = out.shape[:2]
    h = (int(point_size) + 1) // 2
    for px, py in scale_points(pts, scaling).tolist():
        out[max(py - h, 0):max(min(py + h, rows), 0), max(px - h, 0):max(min(px + h, cols), 0)] = colour
    return out


def rect_mask(rows, cols, rect, thickness):
    """The pixels draw_rect sets, as a boolean [rows, cols]."""
    x, y, w, h = (int(v) for v in rect)
    t = int(thickness)
    if t == 0 or w <= 0 or h <= 0:
        raise ValueError("thickness != 0 and a rectangle that is not empty")
    x0, y0, x1, y1 = x, y, x + w - 1, y + h - 1
    yy, xx = np.mgrid[0:rows, 0:cols]
    if t < 0:                                                                   # cv::FILLED
        return (xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1)
    a, b = t // 2, (t - 1) // 2
    outer = (xx >= x0 - a) & (xx <= x1 + b) & (yy >= y0 - a) & (yy <= y1 + b)
    inner = (xx > x0 + b) & (xx < x1 - a) & (yy > y0 + b) & (yy < y1 - a)
    return outer & ~inner


def rect(img, rect_xywh, colour, thickness=2):
    out = _frame(img)
    out[rect_mask(out.shape[0], out.shape[1], rect_xywh, thickness)] = colour
    return out


def _growth(thickness):
    return (int(thickness) - 1) // 2


def _text_args(text, scale, thickness):
    b = text_bytes(text)
    if not (1 <= scale <= MAX_SCALE and 1 <= thickness <= MAX_THICKNESS):
        raise ValueError("1 <= scale <= %d and 1 <= thickness <= %d" % (MAX_SCALE, MAX_THICKNESS))
    return b, int(scale), _growth(thickness)


def text_size(text, scale=3, thickness=2):
    """((width, height), baseline) of the drawn box: n cells less the last one's blank column, seven glyph rows, grown by the thickness; the
    baseline is what the cell keeps below the origin (its blank row, plus the growth)."""
    b, s, g = _text_args(text, scale, thickness)
    w = (CELL_W * len(b) - 1) * s + 2 * g if b else 0
    return (w, GLYPH_H * s + 2 * g), s + g


def text_mask(rows, cols, text, pos, scale, thickness):
    """The pixels draw_text sets: font pixel (c, r) of character i is the block [x + (6 i + c) s, + s) x [y - (7 - r) s, + s), grown by
    (thickness - 1) / 2 pixels on each side; (x, y) is the bottom-left corner of the baseline."""
    b, s, g = _text_args(text, scale, thickness)
    mask = np.zeros((rows, cols), bool)
    if not b:
        return mask
    x, y = int(pos[0]), int(pos[1])
    bits = np.zeros((GLYPH_H, CELL_W * len(b)), bool)
    for i, ch in enumerate(b):
        bits[:, CELL_W * i:CELL_W * i + GLYPH_W] = glyph(ch)
    for r, k in np.argwhere(bits).tolist():
        bx, by = x + k * s, y - (GLYPH_H - r) * s
        mask[max(by - g, 0):max(min(by + s + g, rows), 0), max(bx - g, 0):max(min(bx + s + g, cols), 0)] = True
    return mask


def text(img, string, pos, colour, scale=3, thickness=2):
    out = _frame(img)
    out[text_mask(out.shape[0], out.shape[1], string, pos, scale, thickness)] = colour
    return out


def font_scale_to_scale(font_scale):
    """The facade's mapping of the reference's double font_scale: max(1, cvRound(2 font_scale)) (half to even)."""
    return max(1, int(np.rint(2.0 * float(font_scale))))
