"""FSR 1 EASU scaling (the OBS plugin's FSR filter: FSRFilter / FSREffect, FidelityFX FsrEasuF) over the C-ABI.

Frames are torch uint8 tensors [rows, cols, 3 | 4] on the GPU with contiguous rows (any row pitch: stride(1) == channels, stride(2) == 1).
apply() works out of place on the context's stream; specification: tests/np_fsr.py and DESIGN.md section 16.  apply() also takes GRAY frames
[rows, cols] (lvk_hip_fsr_easu_gray)."""
import ctypes
import math

from . import _native
from .stabilization import CHANNELS, FORMAT_BGR, FORMAT_GRAY, frame_args, gray_frame_args, out_frame

_c = ctypes
MAX_CROP = 4096


def easu_const(rw, rh, W, H, ow, oh):
    """FsrEasuCon's con0 .. con3 (16 float32 values) for a rw x rh viewport of a W x H input scaled to ow x oh (no device needed)."""
    con = (_c.c_float * 16)()
    if _native.load().lvk_hip_fsr_easu_const(int(rw), int(rh), int(W), int(H), int(ow), int(oh), con) != 0:
        raise ValueError("every size must be > 0")
    return list(con)


def fsr_geometry(rows, cols, output_size=None, multiplier=1.0, maintain_aspect_ratio=True, crop=(0, 0, 0, 0)):
    """The region (x, y, w, h), output size (rows, cols) and skip flag of FSRFilter for a rows x cols frame (no device needed).
    output_size = (rows, cols), or None for source x multiplier; crop = (left, top, right, bottom)."""
    oh, ow = (0, 0) if output_size is None else output_size
    region, size, skip = (_c.c_int * 4)(), (_c.c_int * 2)(), _c.c_int()
    rc = _native.load().lvk_hip_fsr_geometry(int(rows), int(cols), int(oh), int(ow), float(multiplier), int(bool(maintain_aspect_ratio)),
                                              (_c.c_int * 4)(*crop), region, size, _c.byref(skip))
    if rc != 0:
        raise ValueError("invalid FSR geometry arguments")
    return tuple(region), tuple(size), bool(skip.value)


class FSRFilter:
    """FSRFilter(ctx, output_size=None, multiplier=1.0, maintain_aspect_ratio=True, crop=(0, 0, 0, 0)).

    output_size = (rows, cols) scales to that size, None scales to the frame's size times `multiplier`; crop = (left, top, right, bottom),
    each in [0, 4096].  A frame the geometry skips is returned as it is."""

    def __init__(self, ctx, output_size=None, multiplier=1.0, maintain_aspect_ratio=True, crop=(0, 0, 0, 0)):
        self.ctx = ctx
        self.lib = ctx.lib
        self.configure(output_size, multiplier, maintain_aspect_ratio, crop)

    def configure(self, output_size=None, multiplier=1.0, maintain_aspect_ratio=True, crop=(0, 0, 0, 0)):
        multiplier = float(multiplier)
        if output_size is not None and (len(output_size) != 2 or min(output_size) < 0):
            raise ValueError("output_size must be (rows, cols) with sizes >= 0")
        if output_size is None and (math.isnan(multiplier) or not 0.0 < multiplier < math.inf):
            raise ValueError("the multiplier must be > 0")
        if len(crop) != 4 or not all(0 <= int(c) <= MAX_CROP for c in crop):
            raise ValueError("crops must lie in [0, 4096]")
        self.output_size = None if output_size is None else (int(output_size[0]), int(output_size[1]))
        self.multiplier = multiplier
        self.maintain_aspect_ratio = bool(maintain_aspect_ratio)
        self.crop = tuple(int(c) for c in crop)

    def geometry(self, rows, cols):
        return fsr_geometry(rows, cols, self.output_size, self.multiplier, self.maintain_aspect_ratio, self.crop)

    def apply(self, frame, fmt=FORMAT_BGR, out=None):
        """Scales `frame` into `out` (a new tensor of the output size when None; it must not overlap `frame`) and returns it.  When the
        geometry skips, `frame` itself is returned (or copied into `out`).  The tensor selects the entry: [rows, cols] is a GRAY frame (`fmt` left
        at its default or FORMAT_GRAY) and `out` is two-dimensional, [rows, cols, 3 | 4] a frame of format `fmt`."""
        gray = frame.dim() == 2
        ch = 1 if gray else CHANNELS.get(fmt)
        if gray and fmt not in (FORMAT_BGR, FORMAT_GRAY):
            raise ValueError("a [rows, cols] frame is a GRAY frame")
        if not gray and ch not in (3, 4):
            raise ValueError("FSR takes BGR / RGB / YUV and BGRA / RGBA frames")
        args = gray_frame_args if gray else (lambda t: frame_args(t, ch))
        src, src_step = args(frame)
        rows, cols = frame.shape[0], frame.shape[1]
        region, (oh, ow), skip = self.geometry(rows, cols)
        if skip:
            if out is None:
                return frame
            if tuple(out.shape) != tuple(frame.shape):
                raise ValueError("out must have the shape of the frame")
            out.copy_(frame)
            return out
        shape = (oh, ow) if gray else (oh, ow, ch)
        out = out_frame(out, frame, shape, "out must have the output shape %r" % (shape,))
        dst, dst_step = args(out)
        reg = (_c.c_int * 4)(*region)
        if gray:
            rc = self.lib.lvk_hip_fsr_easu_gray(self.ctx.handle, src, src_step, rows, cols, reg, dst, dst_step, oh, ow)
        else:
            rc = self.lib.lvk_hip_fsr_easu(self.ctx.handle, src, src_step, rows, cols, int(fmt), reg, dst, dst_step, oh, ow)
        self.ctx._check(rc)
        return out
