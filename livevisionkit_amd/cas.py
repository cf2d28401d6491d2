"""Contrast adaptive sharpening (the OBS plugin's CAS filter: CASFilter / CASEffect, FidelityFX CasFilter) over the C-ABI.

Frames are torch uint8 tensors [rows, cols, 3 | 4] on the GPU with contiguous rows (any row pitch: stride(1) == channels, stride(2) == 1).
apply() works out of place on the context's stream; specification: tests/np_cas.py and DESIGN.md section 14.  apply() also takes GRAY frames
[rows, cols] (lvk_hip_cas_gray)."""
import ctypes
import math

from . import _native
from .stabilization import CHANNELS, FORMAT_BGR, FORMAT_GRAY, frame_args, gray_frame_args, out_frame

_c = ctypes


def cas_const(sharpness):
    """CasSetup's peak weight for a sharpness (float32, no device needed)."""
    peak = _c.c_float()
    if _native.load().lvk_hip_cas_const(float(sharpness), _c.byref(peak)) != 0:
        raise ValueError("sharpness must be a number")
    return peak.value


class CASFilter:
    """CASFilter(ctx, sharpness=0.8): the sharpness lies in [0, 1] (CASEffect::Render asserts it)."""

    def __init__(self, ctx, sharpness=0.8):
        self.ctx = ctx
        self.lib = ctx.lib
        self.configure(sharpness)

    def configure(self, sharpness):
        sharpness = float(sharpness)
        if math.isnan(sharpness) or not 0.0 <= sharpness <= 1.0:
            raise ValueError("sharpness must lie in [0, 1]")
        self.sharpness = sharpness

    def apply(self, frame, fmt=FORMAT_BGR, out=None):
        """Sharpens `frame` into `out` (a new tensor when None; it must not overlap `frame`); returns `out`.  The tensor selects the entry:
        [rows, cols] is a GRAY frame (`fmt` left at its default or FORMAT_GRAY) and `out` is two-dimensional, [rows, cols, 3 | 4] a frame of
        format `fmt`."""
        if frame.dim() == 2:
            if fmt not in (FORMAT_BGR, FORMAT_GRAY):
                raise ValueError("a [rows, cols] frame is a GRAY frame")
            src, src_step = gray_frame_args(frame)
            out = out_frame(out, frame, tuple(frame.shape), "out must have the shape of the frame")
            dst, dst_step = gray_frame_args(out)
            self.ctx._check(self.lib.lvk_hip_cas_gray(self.ctx.handle, src, src_step, frame.shape[0], frame.shape[1], dst, dst_step, self.sharpness))
            return out
        ch = CHANNELS.get(fmt)
        if ch not in (3, 4):
            raise ValueError("CAS takes BGR / RGB / YUV and BGRA / RGBA frames")
        src, src_step = frame_args(frame, ch)
        rows, cols = frame.shape[0], frame.shape[1]
        out = out_frame(out, frame, (rows, cols, ch), "out must have the shape of the frame")
        dst, dst_step = frame_args(out, ch)
        self.ctx._check(self.lib.lvk_hip_cas(self.ctx.handle, src, src_step, rows, cols, int(fmt), dst, dst_step, self.sharpness))
        return out
