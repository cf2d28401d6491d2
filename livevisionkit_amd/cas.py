"""Contrast adaptive sharpening (the OBS plugin's CAS filter: CASFilter / CASEffect, FidelityFX CasFilter) over the C-ABI.

Frames are torch uint8 tensors [rows, cols, 3 | 4] on the GPU with contiguous rows (any row pitch: stride(1) == channels, stride(2) == 1).
apply() works out of place on the context's stream; specification: tests/np_cas.py and DESIGN.md section 14."""
import ctypes
import math

from . import _native
from .stabilization import FORMAT_BGR

_c = ctypes
_CHANNELS = {0: 3, 2: 3, 4: 3, 1: 4, 3: 4}      # LVK_FORMAT_BGR, _RGB, _YUV; _BGRA, _RGBA


def cas_const(sharpness):
    """CasSetup's peak weight for a sharpness (float32, no device needed)."""
    peak = _c.c_float()
    if _native.load().lvk_hip_cas_const(float(sharpness), _c.byref(peak)) != 0:
        raise ValueError("sharpness must be a number")
    return peak.value


def _frame_args(frame, channels):
    if (frame.dim() != 3 or frame.shape[2] != channels or frame.stride(2) != 1 or frame.stride(1) != channels
            or frame.dtype.itemsize != 1):
        raise ValueError("a packed uint8 frame [rows, cols, %d] with contiguous rows is required" % channels)
    return frame.data_ptr(), frame.stride(0)


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
        """Sharpens `frame` into `out` (a new tensor when None; it must not overlap `frame`); returns `out`."""
        import torch
        if fmt not in _CHANNELS:
            raise ValueError("CAS takes BGR / RGB / YUV and BGRA / RGBA frames")
        ch = _CHANNELS[fmt]
        src, src_step = _frame_args(frame, ch)
        rows, cols = frame.shape[0], frame.shape[1]
        if out is None:
            out = torch.empty((rows, cols, ch), dtype=torch.uint8, device=frame.device)
        if tuple(out.shape) != (rows, cols, ch):
            raise ValueError("out must have the shape of the frame")
        dst, dst_step = _frame_args(out, ch)
        self.ctx._check(self.lib.lvk_hip_cas(self.ctx.handle, src, src_step, rows, cols, int(fmt), dst, dst_step, self.sharpness))
        return out
