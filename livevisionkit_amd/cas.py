"""Contrast adaptive sharpening (the OBS plugin's CAS filter: CASFilter / CASEffect, FidelityFX CasFilter) over the C-ABI.

Frames are torch uint8 tensors [rows, cols, 3 | 4] on the GPU with contiguous rows (any row pitch: stride(1) == channels, stride(2) == 1).
apply() works out of place on the context's stream; specification: tests/np_cas.py and DESIGN.md section 14.  apply() also takes GRAY frames
[rows, cols] (lvk_hip_cas_gray).  apply_yuv420 takes the planes of an I420 / NV12 frame and writes new planes
(lvk_hip_cas_yuv420), apply_obs the planes of any OBS video format (lvk_hip_cas_obs)."""
import ctypes
import math

from . import _native
from .context import _planes420_args, _planes420_empty
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

    def apply_yuv420(self, y, u, v=None, out=None):
        """Sharpens the planes of an I420 (y [rows, cols], u, v [rows/2, cols/2]) or NV12 (v=None, u [rows/2, cols/2, 2]) frame OUT OF PLACE in one
        call (lvk_hip_cas_yuv420): byte for byte the ingest -> apply(FORMAT_YUV) -> egress chain.  `out` = the output planes in the same layout
        (allocated when None; rows may be padded: stride(-1) == 1, NV12 UV stride(1) == 2).  Returns the output planes; asynchronous on the context's
        stream."""
        nv12 = v is None
        planes = (y, u) if nv12 else (y, u, v)
        rows, cols = int(y.shape[0]), int(y.shape[1])
        out = _planes420_empty(rows, cols, nv12, y.device) if out is None else tuple(out)
        if len(out) != len(planes):
            raise ValueError("`out` holds one plane per input plane")
        chroma = (rows // 2, cols // 2, 2) if nv12 else (rows // 2, cols // 2)
        shapes = ((rows, cols), chroma) if nv12 else ((rows, cols), chroma, chroma)
        for p, shape in zip(planes + out, shapes * 2):
            if tuple(p.shape) != shape or p.dtype.itemsize != 1 or p.stride(-1) != 1 or (p.dim() == 3 and p.stride(1) != 2):
                raise ValueError("8-bit planes [rows, cols], [rows/2, cols/2] (NV12: [rows/2, cols/2, 2]) with contiguous rows are required")
        self.ctx._check(self.lib.lvk_hip_cas_yuv420(self.ctx.handle, *_planes420_args(planes, nv12), *_planes420_args(out, nv12), rows, cols, 1 if nv12 else 0,
                                                    self.sharpness))
        return out

    def apply_obs(self, fmt, planes, out=None):
        """Sharpens the planes of one frame of ANY OBS video format OUT OF PLACE in one call (lvk_hip_cas_obs): byte for byte the
        ctx.ingest_obs -> apply(the format's frame format) -> ctx.egress_obs chain.  `fmt` = a name of Context.VIDEO_FORMATS or its number; `planes`
        as ctx.ingest_obs takes them; `out` = the planes of the output frame (allocated from the input planes' shapes when None -- bytes the egress
        leaves alone are then undefined; rows may be padded).  Returns the output planes; asynchronous on the context's stream."""
        import torch
        planes = list(planes)
        rows, cols = int(planes[0].shape[0]), int(planes[0].shape[1])
        out = [torch.empty(tuple(p.shape), dtype=torch.uint8, device=p.device) for p in planes] if out is None else list(out)
        if len(out) != len(planes):
            raise ValueError("`out` holds one plane per input plane")
        iptr, istep = self.ctx._obs_args(planes)
        optr, ostep = self.ctx._obs_args(out)
        self.ctx._check(self.lib.lvk_hip_cas_obs(self.ctx.handle, self.ctx.video_format(fmt), iptr, istep, optr, ostep, rows, cols, self.sharpness))
        return out
