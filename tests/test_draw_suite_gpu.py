"""lvk_hip_draw_points / _rect / _text on the GPU against tests/np_draw.py, through livevisionkit_amd.draw_*.  Bar: bit-exact, and not a byte
outside cols * 3 of a row written.  Frames from 1 x 1 to 1080p sit inside a larger buffer of random guard bytes -- before the frame, after every
row (pitches + 1, + 13, + 64), after the frame -- at pointer offsets of 1-3 bytes; the WHOLE buffer is compared, guards included.

draw_points is also pinned to the reference: the `points` kernel of Functions/OpenCL/Sources/Drawing.cl as compiled into
oracle/_ref/drawing.hsaco, launched with the argument list of Functions/Drawing.tpp:127-137 (as tests/test_ref_pin_gpu.py launches `grid` and
`crosses`), on in-frame point sets.  Its loops run over [max(p - w, 0), min(p + w, size)) in both axes (Drawing.cl:55-58), so it writes inside
the frame wherever the point lies; the pin still keeps to in-frame points."""
import ctypes

import numpy as np
import pytest

from tests import np_draw as nd
from tests import ref_cl

pytestmark = pytest.mark.gpu

COLOUR = (7, 200, 99)
HUD = "0.12ms (3.40ms)"
# (rows, cols, extra pitch, pointer offset)
LAYOUTS = [(1, 1, 0, 0), (1, 1, 13, 3), (1, 7, 1, 1), (5, 1, 64, 2), (7, 9, 0, 0), (7, 9, 1, 3), (33, 47, 13, 1), (67, 131, 64, 2), (270, 480, 1, 1),
           (1080, 1920, 0, 0), (1080, 1920, 13, 3)]


class Guarded:
    """A frame inside a buffer of random bytes: `off` bytes in front, `extra` after each row, a tail behind the last row."""

    def __init__(self, rows, cols, extra, off, seed=0):
        import torch
        self.rows, self.cols, self.pitch, self.off = rows, cols, cols * 3 + extra, 64 + off
        self.host = np.random.default_rng(seed + rows * 7 + cols).integers(0, 256, self.off + rows * self.pitch + 256, dtype=np.uint8)
        self.dev = torch.from_numpy(self.host).cuda()
        self.frame = self.dev.as_strided((rows, cols, 3), (self.pitch, 3, 1), self.off)

    def image(self, host=None):
        host = self.host if host is None else host
        return np.lib.stride_tricks.as_strided(host[self.off:], (self.rows, self.cols, 3), (self.pitch, 3, 1)).copy()

    def check(self, ctx, want, what):
        """The buffer now holds `want` in the frame and its old bytes everywhere else; then restores it."""
        ctx.sync()
        expect = self.host.copy()
        np.lib.stride_tricks.as_strided(expect[self.off:], (self.rows, self.cols, 3), (self.pitch, 3, 1))[...] = want
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, expect):
            bad = np.flatnonzero(got != expect)
            rel = bad - self.off
            inside = (rel >= 0) & (rel // self.pitch < self.rows) & (rel % self.pitch < self.cols * 3)
            raise AssertionError(f"{what}: {len(bad)} bytes differ, {int((~inside).sum())} of them outside the frame's rows; first at byte {bad[0]} "
                                 f"(row {rel[0] // self.pitch}, byte {rel[0] % self.pitch} of the row)")
        import torch
        self.dev.copy_(torch.from_numpy(self.host))


def rect_cases(rows, cols):
    r3, c3 = max(rows // 3, 1), max(cols // 3, 1)
    cases = [((cols // 4, rows // 4, max(cols // 2, 1), max(rows // 2, 1)), t) for t in (1, 2, 3, 5, -1)]
    for t in (1, 2, 4):
        cases += [((-3, r3, 8, r3), t), ((cols - 4, r3, 8, r3), t), ((c3, -3, c3, 8), t), ((c3, rows - 4, c3, 8), t),                # each edge
                  ((-2, -2, 6, 6), t), ((cols - 3, -2, 6, 6), t), ((-2, rows - 3, 6, 6), t), ((cols - 3, rows - 3, 6, 6), t)]          # each corner
    cases += [((0, 0, cols, rows), 1), ((0, 0, cols, rows), 3), ((0, 0, cols, rows), -1),                                              # the whole frame
              ((-5, -5, cols + 10, rows + 10), 1), ((-5, -5, cols + 10, rows + 10), 7), ((-5, -5, cols + 10, rows + 10), 12),           # around it
              ((-5, -5, cols + 10, rows + 10), -1), ((cols + 5, 2, 4, 4), 2), ((-50, -50, 10, 10), 3), ((2, rows, 3, 3), 1),            # outside it
              ((cols // 2, rows // 2, 1, 1), 1), ((cols // 2, rows // 2, 1, 1), 2), ((cols // 2, rows // 2, 2, 2), 3), ((0, rows // 2, cols, 1), 1),
              ((-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), 1), ((2 ** 31 - 10, 0, 2 ** 31 - 1, 2 ** 31 - 1), -1), ((-7, -7, 2 ** 31 - 1, 2 ** 31 - 1), 3),
              ((0, 0, 1, 1), 2 ** 31 - 1), ((cols // 2, 0, 1, 1), 9), ((-2 ** 31, 1, 2 ** 31 - 1, 2), -2 ** 31)]
    return cases


@pytest.mark.parametrize("rows,cols,extra,off", LAYOUTS)
def test_rect_bit_exact(ctx, rows, cols, extra, off):
    import livevisionkit_amd as lvk
    g = Guarded(rows, cols, extra, off)
    img = g.image()
    cases = rect_cases(rows, cols)
    if rows * cols > 500000:
        cases = cases[::3]                                          # (every third case at 1080p: the specification's masks take the time)
    drawn = 0
    for rect, t in cases:
        want = nd.rect(img, rect, COLOUR, t)
        drawn += int(not np.array_equal(want, img))
        lvk.draw_rect(ctx, g.frame, rect, COLOUR, t)
        g.check(ctx, want, f"rect {rect} thickness {t}")
    assert drawn >= len(cases) // 3


def point_sets(rows, cols, rng):
    pts = np.c_[rng.uniform(-20, 500, 2000), rng.uniform(-20, 290, 2000)].astype(np.float32)
    pts[:10] = [(0, 0), (480, 270), (479.5, 269.5), (0.5, 1.5), (2.5, 3.5), (1e9, 3), (-1e9, -1e9), (np.nan, 5), (3e38, 3e38), (-0.49, 270.49)]
    return pts, (cols / 480.0, rows / 270.0)


@pytest.mark.parametrize("rows,cols,extra,off", LAYOUTS)
def test_points_bit_exact(ctx, rows, cols, extra, off):
    import livevisionkit_amd as lvk
    g = Guarded(rows, cols, extra, off)
    img = g.image()
    pts, scaling = point_sets(rows, cols, np.random.default_rng(cols))
    for size in (10, 1, 2, 7, 64):
        lvk.draw_points(ctx, g.frame, pts, COLOUR, size, scaling)
        g.check(ctx, nd.points(img, pts, COLOUR, size, scaling), f"2 000 points of size {size}")
    corners = [(0, 0), (cols, rows), (cols - 1, rows - 1), (0, rows), (cols, 0), (cols / 2.0, -1), (-1, rows / 2.0), (cols + 1, rows + 1)]
    for size in (1, 3, 4):
        for p in corners:
            lvk.draw_points(ctx, g.frame, [p], COLOUR, size)
            g.check(ctx, nd.points(img, [p], COLOUR, size), f"point {p} of size {size}")
    lvk.draw_points(ctx, g.frame, [(cols // 2, rows // 2)], COLOUR, 2 ** 31 - 1)              # (one square over the whole frame)
    g.check(ctx, nd.points(img, [(cols // 2, rows // 2)], COLOUR, 2 ** 31 - 1), "a point of the largest size")
    lvk.draw_points(ctx, g.frame, np.zeros((0, 2), np.float32), COLOUR, 10)
    g.check(ctx, img, "no points")


@pytest.mark.parametrize("rows,cols,extra,off", LAYOUTS)
def test_text_clipped_at_each_edge(ctx, rows, cols, extra, off):
    import livevisionkit_amd as lvk
    g = Guarded(rows, cols, extra, off)
    img = g.image()
    (w, h), _ = nd.text_size(HUD, 3, 2)
    places = [(5, 40), (-30, 30), (cols - 40, 30), (10, 5), (10, rows + 8), (cols - w, rows), (-w + 1, h), (cols - 1, rows + h - 1),      # inside, each edge, flush
              (-w, 30), (cols, 30), (10, 0), (10, rows + h), (-5000, 10), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, -2 ** 31)]                 # wholly outside
    drawn = 0
    for scale, thickness in ((3, 2), (1, 1), (2, 3), (5, 6)):
        for pos in places:
            want = nd.text(img, HUD, pos, COLOUR, scale, thickness)
            drawn += int(not np.array_equal(want, img))
            lvk.draw_text(ctx, g.frame, HUD, pos, COLOUR, scale, thickness)
            g.check(ctx, want, f"text at {pos} scale {scale} thickness {thickness}")
    assert drawn >= 2
    lvk.draw_text(ctx, g.frame, "", (5, 40), COLOUR)
    g.check(ctx, img, "the empty string")
    lvk.draw_text(ctx, g.frame, "W", (0, rows), COLOUR, nd.MAX_SCALE, nd.MAX_THICKNESS)       # (the largest block: its first font pixel covers the frame)
    g.check(ctx, nd.text(img, "W", (0, rows), COLOUR, nd.MAX_SCALE, nd.MAX_THICKNESS), "the largest scale and thickness")


@pytest.mark.parametrize("scale", [1, 2, 3, 4])
@pytest.mark.parametrize("thickness", [1, 2, 3])
def test_every_glyph_bit_exact(ctx, scale, thickness):
    """The library's font table against the specification's own copy: all 95 printable glyphs, and bytes outside the range as '?'."""
    import livevisionkit_amd as lvk
    printable = bytes(range(0x20, 0x7F))
    other = bytes([0x01, 0x1F, 0x7F, 0x80, 0xC3, 0xFF]) + "é".encode("utf-8")
    (w, h), baseline = nd.text_size(printable, scale, thickness)
    g = Guarded(2 * (nd.CELL_H * scale + 4) + 3, w + 9, 13, 1, seed=scale * 10 + thickness)
    img = g.image()
    want = img
    for line, text in enumerate((printable, other)):
        pos = (4, (line + 1) * (nd.CELL_H * scale + 4))
        want = nd.text(want, text, pos, COLOUR, scale, thickness)
        lvk.draw_text(ctx, g.frame, text, pos, COLOUR, scale, thickness)
    g.check(ctx, want, f"every glyph at scale {scale} thickness {thickness}")
    assert lvk.text_size(printable, scale, thickness) == ((w, h), baseline)


def test_a_256_byte_string_in_one_call(ctx):
    import livevisionkit_amd as lvk
    text = bytes((0x21 + i % 94) for i in range(256))
    g = Guarded(20, 256 * 6 + 11, 1, 2)
    img = g.image()
    lvk.draw_text(ctx, g.frame, text, (3, 15), COLOUR, 1, 1)
    g.check(ctx, nd.text(img, text, (3, 15), COLOUR, 1, 1), "256 bytes")


def test_refused_calls_leave_the_frame_untouched(ctx):
    import livevisionkit_amd as lvk
    g = Guarded(33, 47, 13, 1)
    img = g.image()
    lib, f = ctx.lib, g.frame
    colour = (ctypes.c_uint8 * 3)(*COLOUR)
    pts = (ctypes.c_float * 2)(5.0, 5.0)
    rect = (ctypes.c_int * 4)(2, 2, 8, 8)
    frame = (ctx.handle, f.data_ptr(), g.pitch, g.rows, g.cols)
    refused = [
        lib.lvk_hip_draw_points(*frame, pts, 1, 1.0, 1.0, colour, 0),
        lib.lvk_hip_draw_points(*frame, pts, 1, 1.0, 1.0, colour, -4),
        lib.lvk_hip_draw_points(*frame, pts, 1, -1.0, 1.0, colour, 3),
        lib.lvk_hip_draw_points(*frame, pts, 1, 1.0, -0.5, colour, 3),
        lib.lvk_hip_draw_points(*frame, pts, 1, float("nan"), 1.0, colour, 3),
        lib.lvk_hip_draw_points(*frame, None, 1, 1.0, 1.0, colour, 3),
        lib.lvk_hip_draw_points(*frame, pts, -1, 1.0, 1.0, colour, 3),
        lib.lvk_hip_draw_points(*frame, pts, 1, 1.0, 1.0, None, 3),
        lib.lvk_hip_draw_points(ctx.handle, None, g.pitch, g.rows, g.cols, pts, 1, 1.0, 1.0, colour, 3),
        lib.lvk_hip_draw_points(ctx.handle, f.data_ptr(), g.cols * 3 - 1, g.rows, g.cols, pts, 1, 1.0, 1.0, colour, 3),
        lib.lvk_hip_draw_rect(*frame, rect, colour, 0),
        lib.lvk_hip_draw_rect(*frame, (ctypes.c_int * 4)(2, 2, 0, 8), colour, 1),
        lib.lvk_hip_draw_rect(*frame, (ctypes.c_int * 4)(2, 2, 8, -1), colour, -1),
        lib.lvk_hip_draw_rect(*frame, None, colour, 1),
        lib.lvk_hip_draw_rect(*frame, rect, None, 1),
        lib.lvk_hip_draw_rect(ctx.handle, f.data_ptr(), g.pitch, 0, g.cols, rect, colour, 1),
        lib.lvk_hip_draw_rect(ctx.handle, f.data_ptr(), g.cols * 3 - 1, g.rows, g.cols, rect, colour, 1),
        lib.lvk_hip_draw_text(*frame, b"a" * 257, 2, 20, colour, 1, 1),
        lib.lvk_hip_draw_text(*frame, b"a", 2, 20, colour, 0, 1),
        lib.lvk_hip_draw_text(*frame, b"a", 2, 20, colour, -2, 1),
        lib.lvk_hip_draw_text(*frame, b"a", 2, 20, colour, 1, 0),
        lib.lvk_hip_draw_text(*frame, b"a", 2, 20, colour, nd.MAX_SCALE + 1, 1),
        lib.lvk_hip_draw_text(*frame, b"a", 2, 20, colour, 1, nd.MAX_THICKNESS + 1),
        lib.lvk_hip_draw_text(*frame, None, 2, 20, colour, 1, 1),
        lib.lvk_hip_draw_text(*frame, b"a", 2, 20, None, 1, 1),
        lib.lvk_hip_draw_text(ctx.handle, f.data_ptr(), g.pitch, g.rows, -3, b"a", 2, 20, colour, 1, 1),
        lib.lvk_hip_draw_points(None, f.data_ptr(), g.pitch, g.rows, g.cols, pts, 1, 1.0, 1.0, colour, 3),
    ]
    assert refused == [-1] * len(refused), refused
    g.check(ctx, img, "refused calls")
    for call in (lambda: lvk.draw_rect(ctx, f, (2, 2, 8, 8), COLOUR, 0), lambda: lvk.draw_points(ctx, f, [(1, 1)], COLOUR, 0),
                 lambda: lvk.draw_text(ctx, f, "a" * 257, (2, 20), COLOUR)):
        with pytest.raises(lvk.LvkHipError):
            call()
    with pytest.raises(ValueError):
        lvk.draw_rect(ctx, f[:, :, :2], (2, 2, 8, 8), COLOUR)                  # not a packed 8UC3 frame
    g.check(ctx, img, "refused calls of the Python mirror")
    lvk.draw_rect(ctx, f, (2, 2, 8, 8), COLOUR, 1)                                # the context still works
    g.check(ctx, nd.rect(img, (2, 2, 8, 8), COLOUR, 1), "a call after the refused ones")


# ---- the reference's own `points` kernel ---------------------------------------------------------------------------------------------------
def _ref_points(ref, dst, points_i32, point_size, colour):
    """Functions/Drawing.tpp:127-137: ReadOnly(points) = (ptr, step, offset, rows, cols), WriteOnly(dst) = (ptr, step, offset, rows, cols),
    (point_size + 1) / 2, Vec4b; one work-item a point."""
    rows, cols = dst.shape[:2]
    n = points_i32.shape[0]
    ref._launch(ref._fn("draw", "points"), (n + 63) // 64, 1, 64, 1, [
        ref._ptr(points_i32), 8, 0, n, 1, ref._ptr(dst), dst.stride(0), 0, rows, cols, (int(point_size) + 1) // 2, ref._bg(colour)])
    return dst


@pytest.mark.parametrize("rows,cols", [(270, 480), (67, 131), (1080, 1920)])
def test_points_equal_the_reference_kernel(ctx, rows, cols):
    import torch
    import livevisionkit_amd as lvk
    if not ref_cl.available():
        pytest.skip("oracle/_ref was not built (`make -C oracle ref` needs the reference's sources)")
    ref = ref_cl.RefKernels()
    rng = np.random.default_rng(rows)
    base = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    # in-frame points in a 240 x 135 coordinate space, the frame's corners among them
    pts = np.c_[rng.uniform(0, 239.9, 600), rng.uniform(0, 134.9, 600)].astype(np.float32)
    pts[:5] = [(0, 0), (239.75, 134.75), (0.5, 1.5), (1.5, 2.5), (120, 67.5)]
    scaling = (float(np.float32(cols) / np.float32(240)), float(np.float32(rows) / np.float32(135)))
    pi = nd.scale_points(pts, scaling)
    keep = (pi[:, 0] >= 0) & (pi[:, 0] < cols) & (pi[:, 1] >= 0) & (pi[:, 1] < rows)
    pts, pi = pts[keep], pi[keep].astype(np.int32)
    assert len(pts) > 500
    for size in (10, 1, 7):
        big = torch.zeros((rows + 64, cols + 64, 3), dtype=torch.uint8, device="cuda")       # (a margin around the reference's target, as for `crosses`)
        a = big[:rows, :cols]
        a.copy_(torch.from_numpy(base))
        _ref_points(ref, a, torch.from_numpy(pi).cuda(), size, COLOUR)
        torch.cuda.synchronize()
        got = lvk.draw_points(ctx, torch.from_numpy(base).cuda(), pts, COLOUR, size, scaling)
        ctx.sync()
        assert np.array_equal(got.cpu().numpy(), a.cpu().numpy()), f"size {size}: HIP vs the reference kernel"
        assert np.array_equal(nd.points(base, pts, COLOUR, size, scaling), a.cpu().numpy()), f"size {size}: specification vs the reference kernel"
        assert not big[rows:].any() and not big[:, cols:].any()
