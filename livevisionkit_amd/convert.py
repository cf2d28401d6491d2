"""Format conversion (the reference's VideoFrame::reformatTo and ConversionFilter, i.e. OpenCV's 8-bit cvtColor) over the C-ABI.

Frames are torch uint8 tensors [rows, cols, C] on the GPU, C = 1 (GRAY), 3 (BGR / RGB / YUV) or 4 (BGRA / RGBA), with contiguous rows (any
row pitch: stride(1) == C, stride(2) == 1).  Both work out of place on the context's stream; specification: tests/np_convert.py and
DESIGN.md section 15."""
import ctypes

from . import _native
from .stabilization import CHANNELS, FORMAT_BGR, frame_args, out_frame

_c = ctypes

# cv::ColorConversionCodes (OpenCV's values) that ConversionFilter takes
COLOR_BGR2BGRA = COLOR_RGB2RGBA = 0
COLOR_BGRA2BGR = COLOR_RGBA2RGB = 1
COLOR_BGR2RGBA = COLOR_RGB2BGRA = 2
COLOR_RGBA2BGR = COLOR_BGRA2RGB = 3
COLOR_BGR2RGB = COLOR_RGB2BGR = 4
COLOR_BGRA2RGBA = COLOR_RGBA2BGRA = 5
COLOR_BGR2GRAY, COLOR_RGB2GRAY = 6, 7
COLOR_GRAY2BGR = COLOR_GRAY2RGB = 8
COLOR_GRAY2BGRA = COLOR_GRAY2RGBA = 9
COLOR_BGRA2GRAY, COLOR_RGBA2GRAY = 10, 11
COLOR_BGR2YUV, COLOR_RGB2YUV, COLOR_YUV2BGR, COLOR_YUV2RGB = 82, 83, 84, 85


def code_target(code, src_fmt, dcn=0):
    """The format cvtColor(code, dcn) makes of a src_fmt frame, or -1 when the combination is refused (no device needed)."""
    return _native.load().lvk_hip_cvt_code_target(int(code), int(src_fmt), int(dcn))


def reformat(ctx, frame, src_fmt, dst_fmt, out=None):
    """VideoFrame::reformatTo: `frame` (format src_fmt) converted to dst_fmt into `out` (a new tensor when None; it must not overlap
    `frame`); returns `out`.  The same format on both sides is a copy."""
    if src_fmt not in CHANNELS or dst_fmt not in CHANNELS:
        raise ValueError("formats are FORMAT_BGR .. FORMAT_GRAY")
    src, src_step = frame_args(frame, CHANNELS[src_fmt])
    rows, cols, dc = frame.shape[0], frame.shape[1], CHANNELS[dst_fmt]
    out = out_frame(out, frame, (rows, cols, dc), "out must be [rows, cols, %d]" % dc)
    dst, dst_step = frame_args(out, dc)
    ctx._check(ctx.lib.lvk_hip_reformat(ctx.handle, src, src_step, rows, cols, int(src_fmt), dst, dst_step, int(dst_fmt)))
    return out


class ConversionFilter:
    """ConversionFilter(ctx, code, output_channels=None): cvtColor(code, output_channels or 0) of the frames it is given."""

    def __init__(self, ctx, code=COLOR_BGR2YUV, output_channels=None):
        self.ctx = ctx
        self.configure(code, output_channels)

    def configure(self, code, output_channels=None):
        dcn = 0 if output_channels is None else int(output_channels)
        if not any(code_target(code, f, dcn) >= 0 for f in CHANNELS):
            raise ValueError("unsupported conversion code %r with %r output channels" % (code, output_channels))
        self.code, self.output_channels = int(code), output_channels

    def target(self, fmt):
        """The format apply() makes of a `fmt` frame (ValueError when the code does not take it)."""
        to = code_target(self.code, fmt, 0 if self.output_channels is None else int(self.output_channels))
        if to < 0:
            raise ValueError("conversion code %d does not take format %r" % (self.code, fmt))
        return to

    def apply(self, frame, fmt=FORMAT_BGR, out=None):
        """Converts `frame` of format `fmt`; returns (out, destination format)."""
        to = self.target(fmt)
        return reformat(self.ctx, frame, fmt, to, out=out), to
