"""Lens correction (the OBS plugin's LCFilter, Modules/OBS-Plugin/Sources/Enhancement/LCFilter.cpp) over the C-ABI: lvk_hip_lens_* of include/lvk_hip.h,
DESIGN.md section 27.

The filter owns the camera profile (fx, fy, cx, cy, k1, k2, p1, p2, k3), the offset map of the last frame size and the test mode, whose 32 x 32 magenta grid
is drawn before the warp.  Frames are torch uint8 tensors on the GPU with contiguous rows (any row pitch); applies are asynchronous on the context's stream
and out of place.  apply_obs takes the planes of any OBS video format in one call (lvk_hip_lens_apply_obs)."""
import ctypes

from .context import Context, _planes420_args, _planes420_empty
from .stabilization import CHANNELS, FORMAT_BGRA, FORMAT_GRAY, FORMAT_YUV, frame_args, gray_frame_args, out_frame

_c = ctypes


def _profile(profile):
    return None if profile is None else (_c.c_double * 9)(*[float(v) for v in profile])


class LCFilter:
    """LCFilter(profile=None, test_mode=False, context=None): profile = the nine camera parameters, or None for "no profile selected" (frames pass
    through, with the grid in test mode)."""

    def __init__(self, profile=None, test_mode=False, context=None, device=0):
        self.ctx = context if context is not None else Context(device)
        self.lib = self.ctx.lib
        h = _c.c_void_p()
        self.ctx._check(self.lib.lvk_hip_lens_create(self.ctx.handle, _profile(profile), 1 if test_mode else 0, _c.byref(h)))
        self.handle = h
        self.profile, self.test_mode = profile, bool(test_mode)

    def configure(self, profile=None, test_mode=False):
        """Another profile (None: none) and test mode; a profile with fx == 0 or fy == 0 raises and leaves the filter as it was."""
        self.ctx._check(self.lib.lvk_hip_lens_configure(self.handle, _profile(profile), 1 if test_mode else 0))
        self.profile, self.test_mode = profile, bool(test_mode)

    def view(self, rows, cols):
        """The valid-pixel region (x, y, w, h) of a rows x cols frame under the profile; the whole frame without one."""
        v = (_c.c_int * 4)()
        self.ctx._check(self.lib.lvk_hip_lens_view(self.handle, int(rows), int(cols), v))
        return tuple(v)

    def apply(self, frame, fmt=FORMAT_YUV, out=None):
        """Corrects `frame` into `out` (a new tensor when None); returns `out`.  The tensor selects the entry: [rows, cols] is a GRAY frame (`fmt`
        ignored), [rows, cols, 4] a BGRA / RGBA frame (`fmt` FORMAT_BGRA unless it names a four-channel format), [rows, cols, 3] a frame of format
        `fmt`.  In test mode the grid is drawn into `frame` itself before the warp (three channels; one and four channels are refused)."""
        rows, cols = frame.shape[0], frame.shape[1]
        if frame.dim() == 2:
            src, src_step = gray_frame_args(frame)
            out = out_frame(out, frame, (rows, cols), "out must have the shape of the frame")
            dst, dst_step = gray_frame_args(out)
            rc = self.lib.lvk_hip_lens_apply_gray(self.handle, src, src_step, rows, cols, dst, dst_step)
        elif frame.dim() == 3 and frame.shape[2] == 4:
            if CHANNELS.get(fmt) != 4:
                fmt = FORMAT_BGRA
            src, src_step = frame_args(frame, 4)
            out = out_frame(out, frame, (rows, cols, 4), "out must have the shape of the frame")
            dst, dst_step = frame_args(out, 4)
            rc = self.lib.lvk_hip_lens_apply_c4(self.handle, src, src_step, rows, cols, int(fmt), dst, dst_step)
        else:
            if fmt == FORMAT_GRAY:
                raise ValueError("a GRAY frame is [rows, cols]")
            src, src_step = frame_args(frame, 3)
            out = out_frame(out, frame, (rows, cols, 3), "out must have the shape of the frame")
            dst, dst_step = frame_args(out, 3)
            rc = self.lib.lvk_hip_lens_apply(self.handle, src, src_step, rows, cols, int(fmt), dst, dst_step)
        self.ctx._check(rc)
        return out

    def apply_yuv420(self, y, u, v=None, out=None):
        """The planes of an I420 (y [rows, cols], u, v [rows/2, cols/2]) or NV12 (v=None, u [rows/2, cols/2, 2]) frame in one call
        (lvk_hip_lens_apply_yuv420): byte for byte ingest_yuv420 -> [draw_grid] -> remap_map(yuv=True, bg 0) -> egress_yuv420.  `out` = the output
        planes in the same layout (allocated when None).  Returns them."""
        nv12 = v is None
        planes = (y, u) if nv12 else (y, u, v)
        rows, cols = int(y.shape[0]), int(y.shape[1])
        out = _planes420_empty(rows, cols, nv12, y.device) if out is None else tuple(out)
        if len(out) != len(planes):
            raise ValueError("`out` holds one plane per input plane")
        self.ctx._check(self.lib.lvk_hip_lens_apply_yuv420(self.handle, *_planes420_args(planes, nv12), *_planes420_args(out, nv12), rows, cols, 1 if nv12 else 0))
        return out

    @staticmethod
    def obs_plane_shapes(fmt, rows, cols):
        """The planes of one rows x cols frame of `fmt` (a name): StabilizationFilter.obs_plane_shapes, and the one plane of Y800."""
        from .stabilization import StabilizationFilter
        return [(rows, cols)] if fmt == "Y800" else StabilizationFilter.obs_plane_shapes(fmt, rows, cols)

    def apply_obs(self, fmt, planes, out=None):
        """The planes of one frame of ANY OBS video format in one call (lvk_hip_lens_apply_obs): byte for byte ingest_obs -> [draw_grid] ->
        [remap_map(bg 0)] -> egress_obs.  `fmt` = a name of Context.VIDEO_FORMATS or its number; `planes` as Context.ingest_obs takes them, in the shapes
        of obs_plane_shapes; `out` = planes of the same shapes (allocated when None: bytes the egress leaves alone are then undefined).  Returns `out`.
        Y800 is refused in test mode."""
        import torch
        planes = list(planes)
        rows, cols = int(planes[0].shape[0]), int(planes[0].shape[1])
        out = [torch.empty(tuple(p.shape), dtype=torch.uint8, device=p.device) for p in planes] if out is None else list(out)
        if len(out) != len(planes):
            raise ValueError("`out` holds one plane per input plane")
        iptr, istep = self.ctx._obs_args(planes)
        optr, ostep = self.ctx._obs_args(out)
        self.ctx._check(self.lib.lvk_hip_lens_apply_obs(self.handle, self.ctx.video_format(fmt), iptr, istep, optr, ostep, rows, cols))
        return out

    def close(self):
        # (a filter that outlives its context must not hand a dangling context to the library: the handle is dropped)
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):
                self.lib.lvk_hip_lens_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
