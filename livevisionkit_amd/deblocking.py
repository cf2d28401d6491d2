"""Host-side mirror of lvk::DeblockingFilter (reference: LiveVisionKit/Filters/DeblockingFilter.hpp:26-57) over the C-ABI.
Same method names: configure / apply / draw_influence / filter_region.  Frames are torch uint8 tensors [rows, cols, 3] on the GPU
(any row pitch: a view with stride(1) == 3 and stride(2) == 1), filtered IN PLACE like the reference's apply(frame, frame).  apply also takes
GRAY frames [rows, cols] and BGRA / RGBA frames [rows, cols, 4] (lvk_hip_deblock_apply_gray / _c4).  apply_yuv420 takes the planes of an I420 / NV12
frame and writes new planes (lvk_hip_deblock_apply_yuv420), apply_obs the planes of any OBS video format (lvk_hip_deblock_apply_obs)."""
import ctypes

import numpy as np

from . import _native
from .context import _planes420_args, _planes420_empty
from .stabilization import FORMAT_YUV, frame_args

_c = ctypes


class DeblockingFilterSettings(_c.Structure):
    """lvk::DeblockingFilterSettings (field-for-field lvk_deblock_settings of include/lvk_hip.h)."""
    _fields_ = [("detection_levels", _c.c_uint32), ("block_size", _c.c_uint32), ("filter_size", _c.c_uint32), ("filter_scaling", _c.c_float)]

    def __init__(self, **over):
        super().__init__()
        _native.load().lvk_hip_deblock_default_settings(_c.byref(self))
        for k, v in over.items():
            setattr(self, k, v)


def _frame_args(frame):
    return (*frame_args(frame, 3, "8UC3"), frame.shape[0], frame.shape[1])


class DeblockingFilter:
    """DeblockingFilter(ctx, **settings): settings by name (detection_levels, block_size, filter_size, filter_scaling) or settings=..."""

    def __init__(self, ctx, settings=None, **over):
        self.ctx = ctx
        self.lib = ctx.lib
        s = settings if settings is not None else DeblockingFilterSettings(**over)
        handle = _c.c_void_p()
        ctx._check(self.lib.lvk_hip_deblock_create(ctx.handle, _c.byref(s), _c.byref(handle)))
        self.handle = handle
        self.settings = s

    def configure(self, settings=None, **over):
        s = settings if settings is not None else DeblockingFilterSettings(**over)
        self.ctx._check(self.lib.lvk_hip_deblock_configure(self.handle, _c.byref(s)))
        self.settings = s

    def apply(self, frame, fmt=FORMAT_YUV):
        """Deblocks `frame` in place (asynchronous on the context's stream); returns the filter region (x, y, w, h).  The tensor selects the
        entry: [rows, cols] is a GRAY frame (`fmt` ignored), [rows, cols, 4] with stride(1) == 4 a BGRA / RGBA frame of format `fmt`, anything
        else goes to the three-channel entry with `fmt` (which refuses GRAY / BGRA / RGBA there)."""
        region = (_c.c_int * 4)()
        if frame.dim() == 2:
            if frame.stride(1) != 1 or frame.dtype.itemsize != 1:
                raise ValueError("a packed 8UC1 frame [rows, cols] with contiguous rows is required")
            rc = self.lib.lvk_hip_deblock_apply_gray(self.handle, frame.data_ptr(), frame.stride(0), frame.shape[0], frame.shape[1], region)
        elif frame.dim() == 3 and frame.shape[2] == 4:
            rc = self.lib.lvk_hip_deblock_apply_c4(self.handle, *frame_args(frame, 4, "8UC4"), frame.shape[0], frame.shape[1], int(fmt), region)
        else:
            rc = self.lib.lvk_hip_deblock_apply(self.handle, *_frame_args(frame), int(fmt), region)
        self.ctx._check(rc)
        return tuple(region)

    def apply_yuv420(self, y, u, v=None, out=None):
        """Deblocks the planes of an I420 (y [rows, cols], u, v [rows/2, cols/2]) or NV12 (v=None, u [rows/2, cols/2, 2]) frame OUT OF PLACE in one
        call (lvk_hip_deblock_apply_yuv420): byte for byte the ingest -> apply(FORMAT_YUV) -> egress chain.  `out` = the output planes in the same
        layout (allocated when None; rows may be padded: stride(-1) == 1, NV12 UV stride(1) == 2).  Returns (planes, region); asynchronous on the
        context's stream."""
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

        region = (_c.c_int * 4)()
        self.ctx._check(self.lib.lvk_hip_deblock_apply_yuv420(self.handle, *_planes420_args(planes, nv12), *_planes420_args(out, nv12), 1 if nv12 else 0, rows, cols, region))
        return out, tuple(region)

    def apply_obs(self, fmt, planes, out=None):
        """Deblocks the planes of one frame of ANY OBS video format OUT OF PLACE in one call (lvk_hip_deblock_apply_obs): byte for byte the
        ctx.ingest_obs -> apply(the format's frame format) -> ctx.egress_obs chain.  `fmt` = a name of Context.VIDEO_FORMATS or its number; `planes`
        as ctx.ingest_obs takes them; `out` = the planes of the output frame (allocated from the input planes' shapes when None -- bytes the egress
        leaves alone are then undefined; rows may be padded).  Returns (planes, region); asynchronous on the context's stream."""
        import torch
        planes = list(planes)
        rows, cols = int(planes[0].shape[0]), int(planes[0].shape[1])
        out = [torch.empty(tuple(p.shape), dtype=torch.uint8, device=p.device) for p in planes] if out is None else list(out)
        if len(out) != len(planes):
            raise ValueError("`out` holds one plane per input plane")
        iptr, istep = self.ctx._obs_args(planes)
        optr, ostep = self.ctx._obs_args(out)
        region = (_c.c_int * 4)()
        self.ctx._check(self.lib.lvk_hip_deblock_apply_obs(self.handle, self.ctx.video_format(fmt), iptr, istep, optr, ostep, rows, cols, region))
        return out, tuple(region)

    def draw_influence(self, frame, fmt=FORMAT_YUV):
        self.ctx._check(self.lib.lvk_hip_deblock_draw_influence(self.handle, *_frame_args(frame), int(fmt)))

    def filter_region(self):
        region = (_c.c_int * 4)()
        self.ctx._check(self.lib.lvk_hip_deblock_filter_region(self.handle, region))
        return tuple(region)

    def grid(self):
        """Diagnostics tap: (mean, grid, keep_block) of the last apply as [ey, ex] numpy arrays (synchronises the stream)."""
        ext = (_c.c_int * 2)()
        x, y, w, h = self.filter_region()
        bs = int(self.settings.block_size) or 1
        cap = max(1, (w // bs) * (h // bs))
        while True:
            mean = np.zeros(cap, np.uint8); grid = np.zeros(cap, np.uint8); keep = np.zeros(cap, np.float32)
            n = self.lib.lvk_hip_deblock_get_grid(self.handle, mean.ctypes.data_as(_c.POINTER(_c.c_uint8)), grid.ctypes.data_as(_c.POINTER(_c.c_uint8)),
                                                  keep.ctypes.data_as(_c.POINTER(_c.c_float)), cap, ext)
            if n >= 0 or ext[0] * ext[1] <= cap:
                break
            cap = ext[0] * ext[1]          # configured to another block size since the last apply
        self.ctx._check(min(n, 0))
        shape = (ext[1], ext[0])
        return mean[:n].reshape(shape), grid[:n].reshape(shape), keep[:n].reshape(shape)

    def close(self):
        # (a filter that outlives its context -- a failed test whose traceback keeps it alive past the session's Context -- must not hand a
        #  dangling context to the library: the handle is dropped, its buffers went with the context's pool)
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):
                self.lib.lvk_hip_deblock_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
