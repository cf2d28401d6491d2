"""The test-mode HUD over the C-ABI: lvk::draw_points, lvk::draw_rect and lvk::draw_text (lvk_hip_draw_points / _rect / _text of lvk_hip.h).

Frames are torch uint8 tensors [rows, cols, 3] on the GPU with contiguous rows (any row pitch); every call draws IN PLACE, asynchronously
on the context's stream, and returns the frame.  The font is this library's own 5 x 7 one, not OpenCV's.  Specification: tests/np_draw.py
and DESIGN.md section 17."""
import ctypes

import numpy as np

from . import _native
from .context import _u8x3
from .stabilization import frame_args

_c = ctypes


def _text_bytes(text):
    b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    if 0 in b:
        raise ValueError("the text is passed as a C string: no NUL byte")
    return b


def draw_points(ctx, frame, points, colour, point_size=10, scaling=(1.0, 1.0)):
    """lvk::draw_points(dst, points, colour, point_size, coord_scaling): squares of half width (point_size + 1) / 2."""
    dst, step = frame_args(frame, 3)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
    ca, cp = _u8x3(colour)
    ctx._check(ctx.lib.lvk_hip_draw_points(ctx.handle, dst, step, frame.shape[0], frame.shape[1], p.ctypes.data_as(_c.POINTER(_c.c_float)), len(p),
                                           float(scaling[0]), float(scaling[1]), cp, int(point_size)))
    return frame


def draw_rect(ctx, frame, rect, colour, thickness=2):
    """lvk::draw_rect(dst, rect = (x, y, w, h), colour, thickness): a band with square corners; thickness < 0 fills."""
    dst, step = frame_args(frame, 3)
    ca, cp = _u8x3(colour)
    r = (_c.c_int * 4)(*[int(v) for v in rect])
    ctx._check(ctx.lib.lvk_hip_draw_rect(ctx.handle, dst, step, frame.shape[0], frame.shape[1], r, cp, int(thickness)))
    return frame


def draw_text(ctx, frame, text, position, colour, scale=3, thickness=2):
    """lvk::draw_text(dst, text, position, colour): position = (x, y) of the baseline's left end; every font pixel is a scale x scale block."""
    dst, step = frame_args(frame, 3)
    ca, cp = _u8x3(colour)
    ctx._check(ctx.lib.lvk_hip_draw_text(ctx.handle, dst, step, frame.shape[0], frame.shape[1], _text_bytes(text), int(position[0]), int(position[1]),
                                         cp, int(scale), int(thickness)))
    return frame


def text_size(text, scale=3, thickness=2):
    """((width, height), baseline) of the box draw_text draws into (no device needed)."""
    wh, baseline = (_c.c_int * 2)(), _c.c_int()
    if _native.load().lvk_hip_text_size(_text_bytes(text), int(scale), int(thickness), wh, _c.byref(baseline)) != 0:
        raise ValueError("text of at most 256 bytes, scale in [1, 32767], thickness in [1, 65535]")
    return (wh[0], wh[1]), baseline.value
