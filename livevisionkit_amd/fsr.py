"""FSR 1 EASU scaling (the OBS plugin's FSR filter: FSRFilter / FSREffect, FidelityFX FsrEasuF) over the C-ABI.

Frames are torch uint8 tensors [rows, cols, 3 | 4] on the GPU with contiguous rows (any row pitch: stride(1) == channels, stride(2) == 1).
apply() works out of place on the context's stream; specification: tests/np_fsr.py and DESIGN.md section 16.  apply() also takes GRAY frames
[rows, cols] (lvk_hip_fsr_easu_gray).  apply_yuv420 takes the planes of an I420 / NV12 frame and writes new planes at the output size
(lvk_hip_fsr_yuv420), apply_obs the planes of any OBS video format (lvk_hip_fsr_obs)."""
import ctypes
import math

from . import _native
from .context import _planes420_args, _planes420_empty
from .stabilization import CHANNELS, FORMAT_BGR, FORMAT_GRAY, frame_args, gray_frame_args, out_frame

_c = ctypes
MAX_CROP = 4096
_FORMATS_420 = (1, 2, 13)              # I420, NV12, I40A: even rows and cols
_FORMATS_422 = (3, 4, 5, 12, 14)       # YVYU, YUY2, UYVY, I422, I42A: even cols


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

    @staticmethod
    def _skipped(planes, out):
        """A frame the geometry skips: the input planes themselves, or copied into `out`."""
        if out is None:
            return planes
        for o, p in zip(out, planes):
            if tuple(o.shape) != tuple(p.shape):
                raise ValueError("out must have the shapes of the input planes")
            o.copy_(p)
        return out

    def apply_yuv420(self, y, u, v=None, out=None):
        """Scales the planes of an I420 (y [rows, cols], u, v [rows/2, cols/2]) or NV12 (v=None, u [rows/2, cols/2, 2]) frame OUT OF PLACE in one call
        (lvk_hip_fsr_yuv420): byte for byte the ingest -> apply(FORMAT_YUV) -> egress chain.  `out` = the output planes in the same layout at the output
        size (allocated when None; rows may be padded: stride(-1) == 1, NV12 UV stride(1) == 2).  An output size with an odd side raises ValueError.
        Returns the output planes as a tuple; a frame the geometry skips comes back as the input planes (or copied into `out`).  Asynchronous on the
        context's stream."""
        nv12 = v is None
        planes = (y, u) if nv12 else (y, u, v)
        rows, cols = int(y.shape[0]), int(y.shape[1])
        if out is not None:
            out = tuple(out)
            if len(out) != len(planes):
                raise ValueError("`out` holds one plane per input plane")
        region, (oh, ow), skip = self.geometry(rows, cols)
        if skip:
            return self._skipped(planes, out)
        if (oh | ow) & 1:
            raise ValueError("a 4:2:0 frame takes even sizes only: the output would be %d x %d" % (ow, oh))
        out = _planes420_empty(oh, ow, nv12, y.device) if out is None else out
        for group, (r, c) in ((planes, (rows, cols)), (out, (oh, ow))):
            chroma = (r // 2, c // 2, 2) if nv12 else (r // 2, c // 2)
            for p, shape in zip(group, ((r, c), chroma, chroma)):
                if tuple(p.shape) != shape or p.dtype.itemsize != 1 or p.stride(-1) != 1 or (p.dim() == 3 and p.stride(1) != 2):
                    raise ValueError("8-bit planes [rows, cols], [rows/2, cols/2] (NV12: [rows/2, cols/2, 2]) with contiguous rows are required")
        self.ctx._check(self.lib.lvk_hip_fsr_yuv420(self.ctx.handle, *_planes420_args(planes, nv12), rows, cols, (_c.c_int * 4)(*region),
                                                    *_planes420_args(out, nv12), oh, ow, 1 if nv12 else 0))
        return out

    def apply_obs(self, fmt, planes, out=None):
        """Scales the planes of one frame of ANY OBS video format OUT OF PLACE in one call (lvk_hip_fsr_obs): byte for byte the
        ctx.ingest_obs -> apply(the format's frame format) -> ctx.egress_obs chain.  `fmt` = a name of Context.VIDEO_FORMATS or its number; `planes`
        as ctx.ingest_obs takes them; `out` = the planes of the output frame at the output size (allocated when None -- plane i is the input's plane i
        at the new size; bytes the egress leaves alone are then undefined; rows may be padded).  An output size the format cannot take (an odd width on
        4:2:2, an odd side on 4:2:0) raises ValueError.  Returns the output planes as a list; a frame the geometry skips comes back as the input planes
        (or copied into `out`).  Asynchronous on the context's stream."""
        import torch
        planes = list(planes)
        vf = self.ctx.video_format(fmt)
        rows, cols = int(planes[0].shape[0]), int(planes[0].shape[1])
        if out is not None:
            out = list(out)
            if len(out) != len(planes):
                raise ValueError("`out` holds one plane per input plane")
        region, (oh, ow), skip = self.geometry(rows, cols)
        if skip:
            return self._skipped(planes, out)
        if (vf in _FORMATS_420 and (oh | ow) & 1) or (vf in _FORMATS_422 and ow & 1):
            raise ValueError("video format %r does not take the output size %d x %d" % (fmt, ow, oh))
        if out is None:
            out = [torch.empty((p.shape[0] * oh // rows, p.shape[1] * ow // cols, *p.shape[2:]), dtype=torch.uint8, device=p.device) for p in planes]
        iptr, istep = self.ctx._obs_args(planes)
        optr, ostep = self.ctx._obs_args(out)
        self.ctx._check(self.lib.lvk_hip_fsr_obs(self.ctx.handle, vf, iptr, istep, rows, cols, (_c.c_int * 4)(*region), optr, ostep, oh, ow))
        return out
