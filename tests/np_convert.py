"""Independent numpy restatement of the reference's format conversion: VideoFrame::reformatTo (Data/VideoFrame.cpp:170-301) and
ConversionFilter (Filters/ConversionFilter.cpp:46-57), i.e. OpenCV 4.8's CPU 8-bit cv::cvtColor paths for the six VideoFrame formats.

Integer arithmetic only.  What was restated, and from where (OpenCV 4.8, modules/imgproc/src):

  byte shuffle  color_rgb.simd.hpp RGB2RGB<uchar>: BGR <-> RGB, BGRA <-> RGBA (alpha kept), 3 -> 4 (alpha = 255), 4 -> 3 (alpha
                dropped), with or without the R / B swap.  Exact.
  -> GRAY       color_rgb.simd.hpp RGB2Gray<uchar>, gray_shift = 15, coefficients R2Y 9798, G2Y 19235, B2Y 3735 (sum 32768):
                gray = (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15.  The tracker's grey (oracle/imgproc.cpp:67-69) is the same.
  -> YUV        color_yuv.simd.hpp RGB2YCrCb_i<uchar> with the YUV coefficients (B2Y 1868, G2Y 9617, R2Y 4899, B2UI 8061, R2VI 14369),
                yuv_shift = 14, delta = 128 << 14, CV_DESCALE(x, n) = (x + (1 << (n - 1))) >> n, saturate_cast<uchar>:
                  Y = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14
                  U = sat(((B - Y) * 8061 + (128 << 14) + 8192) >> 14)
                  V = sat(((R - Y) * 14369 + (128 << 14) + 8192) >> 14)
                The shifts are arithmetic (a negative sum floors, then saturates to 0).  A 4-channel source ignores its alpha.
  YUV ->        color_yuv.simd.hpp YCrCb2RGB_i<uchar> with the YUV coefficients (U2BI 33292, U2GI -6472, V2GI -9519, V2RI 18678):
                  b = sat(Y + (((U - 128) * 33292 + 8192) >> 14))
                  g = sat(Y + (((U - 128) * -6472 + (V - 128) * -9519 + 8192) >> 14))
                  r = sat(Y + (((V - 128) * 18678 + 8192) >> 14))
                alpha = 255 for 4 destination channels (dcn = 4).
  YUV -> GRAY   cv::extractChannel(.., 0) (VideoFrame.cpp:260): Y.
  GRAY ->       GRAY2BGR / GRAY2BGRA (color_rgb.simd.hpp Gray2RGB<uchar>): replicate, alpha 255; GRAY -> YUV is cv::merge(gray, 128, 128)
                (VideoFrame.cpp:278-294).

The dispatch of the 30 ordered pairs is VideoFrame.cpp:186-301 (see PAIRS).  Declared choices:
  1. YUV -> BGRA / RGBA: the reference writes cvtColor(.., dcn = 4) into its step_buffer and leaves dst stale (VideoFrame.cpp:262,264);
     here the destination receives YUV2BGR / YUV2RGB with alpha 255, what cvtColor(.., dcn = 4) computes.
  2. After ConversionFilter the format tag is the code's destination format (the reference keeps the old tag, ConversionFilter.cpp:46-57).
  3. The same format on both sides: reformatTo copies, reformat does nothing, viewAsFormat shares the buffer (VideoFrame.cpp:160-184,303-310).
  4. The reference runs OpenCV's OpenCL cvtColor on a UMat; this specification is the CPU path, as for sections 13 and 14.
"""
import numpy as np

BGR, BGRA, RGB, RGBA, YUV, GRAY = 0, 1, 2, 3, 4, 5
FORMATS = (BGR, BGRA, RGB, RGBA, YUV, GRAY)
NAMES = {BGR: "BGR", BGRA: "BGRA", RGB: "RGB", RGBA: "RGBA", YUV: "YUV", GRAY: "GRAY"}
CHANNELS = {BGR: 3, BGRA: 4, RGB: 3, RGBA: 4, YUV: 3, GRAY: 1}

# OpenCV's cv::ColorConversionCodes values (imgproc.hpp) for the codes ConversionFilter takes
COLOR_BGR2BGRA, COLOR_RGB2RGBA = 0, 0
COLOR_BGRA2BGR, COLOR_RGBA2RGB = 1, 1
COLOR_BGR2RGBA, COLOR_RGB2BGRA = 2, 2
COLOR_RGBA2BGR, COLOR_BGRA2RGB = 3, 3
COLOR_BGR2RGB, COLOR_RGB2BGR = 4, 4
COLOR_BGRA2RGBA, COLOR_RGBA2BGRA = 5, 5
COLOR_BGR2GRAY, COLOR_RGB2GRAY = 6, 7
COLOR_GRAY2BGR, COLOR_GRAY2RGB = 8, 8
COLOR_GRAY2BGRA, COLOR_GRAY2RGBA = 9, 9
COLOR_BGRA2GRAY, COLOR_RGBA2GRAY = 10, 11
COLOR_BGR2YUV, COLOR_RGB2YUV, COLOR_YUV2BGR, COLOR_YUV2RGB = 82, 83, 84, 85

# code -> ({source format: destination format}, destination channels).  The aliased codes take both of their source formats; the BGR / RGB
# -> YUV and -> GRAY codes also take the twin of the other channel count (OpenCV's scn = 3 or 4); YUV2BGR / YUV2RGB also take dcn = 4.
CODES = {
    0: ({BGR: BGRA, RGB: RGBA}, 4),
    1: ({BGRA: BGR, RGBA: RGB}, 3),
    2: ({BGR: RGBA, RGB: BGRA}, 4),
    3: ({RGBA: BGR, BGRA: RGB}, 3),
    4: ({BGR: RGB, RGB: BGR}, 3),
    5: ({BGRA: RGBA, RGBA: BGRA}, 4),
    6: ({BGR: GRAY, BGRA: GRAY}, 1),
    7: ({RGB: GRAY, RGBA: GRAY}, 1),
    8: ({GRAY: BGR}, 3),
    9: ({GRAY: BGRA}, 4),
    10: ({BGRA: GRAY, BGR: GRAY}, 1),
    11: ({RGBA: GRAY, RGB: GRAY}, 1),
    82: ({BGR: YUV, BGRA: YUV}, 3),
    83: ({RGB: YUV, RGBA: YUV}, 3),
    84: ({YUV: BGR}, 3),
    85: ({YUV: RGB}, 3),
}


def code_target(code, src_fmt, dcn):
    """The LVK format cvtColor(code, dcn) makes of a src_fmt frame, or -1 (lvk_hip_cvt_code_target)."""
    if code not in CODES:
        return -1
    table, ch = CODES[code]
    if src_fmt not in table:
        return -1
    if code in (84, 85) and dcn == 4:
        return {84: BGRA, 85: RGBA}[code]
    if dcn not in (0, ch):
        return -1
    return table[src_fmt]


def _sat(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def _bgr_planes(img, fmt):
    """(b, g, r) as int32 planes of a BGR / BGRA / RGB / RGBA frame."""
    x = img.astype(np.int32)
    if fmt in (BGR, BGRA):
        return x[..., 0], x[..., 1], x[..., 2]
    return x[..., 2], x[..., 1], x[..., 0]


def gray_of(b, g, r):
    """RGB2Gray<uchar>: 15-bit fixed point."""
    return ((np.asarray(b, np.int32) * 3735 + np.asarray(g, np.int32) * 19235 + np.asarray(r, np.int32) * 9798 + (1 << 14)) >> 15)


def yuv_of(b, g, r):
    """RGB2YCrCb_i<uchar> with the YUV coefficients: (Y, U, V) as int32, saturated."""
    b, g, r = (np.asarray(v, np.int32) for v in (b, g, r))
    y = (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14
    u = np.clip(((b - y) * 8061 + (128 << 14) + 8192) >> 14, 0, 255)
    v = np.clip(((r - y) * 14369 + (128 << 14) + 8192) >> 14, 0, 255)
    return y, u, v


def bgr_of_yuv(y, u, v, saturate=True):
    """YCrCb2RGB_i<uchar> with the YUV coefficients: (b, g, r) as int32 (saturated unless saturate=False)."""
    y, u, v = (np.asarray(t, np.int32) for t in (y, u, v))
    du, dv = u - 128, v - 128
    b = y + ((du * 33292 + 8192) >> 14)
    g = y + ((du * -6472 + dv * -9519 + 8192) >> 14)
    r = y + ((dv * 18678 + 8192) >> 14)
    if saturate:
        b, g, r = (np.clip(t, 0, 255) for t in (b, g, r))
    return b, g, r


def _pack(fmt, b, g, r, alpha=None):
    """Pack (b, g, r) planes into a BGR / BGRA / RGB / RGBA frame; alpha = 255 unless given."""
    planes = [b, g, r] if fmt in (BGR, BGRA) else [r, g, b]
    if CHANNELS[fmt] == 4:
        planes.append(np.full_like(np.asarray(b), 255) if alpha is None else alpha)
    return _sat(np.stack(planes, axis=-1))


# The dispatch of VideoFrame::reformatTo (VideoFrame.cpp:186-301): (src, dst) -> the operation, as the reference names it
PAIRS = {
    (BGR, GRAY): "BGR2GRAY", (BGR, RGB): "BGR2RGB", (BGR, YUV): "BGR2YUV", (BGR, RGBA): "BGR2RGBA", (BGR, BGRA): "BGR2BGRA",          # :191-197
    (BGRA, GRAY): "BGRA2GRAY", (BGRA, RGB): "BGRA2RGB", (BGRA, BGR): "BGRA2BGR", (BGRA, RGBA): "BGRA2RGBA",                         # :206-209
    (BGRA, YUV): "BGRA2BGR, BGR2YUV",                                                                                                  # :212-216
    (RGB, GRAY): "RGB2GRAY", (RGB, BGR): "RGB2BGR", (RGB, YUV): "RGB2YUV", (RGB, RGBA): "RGB2RGBA", (RGB, BGRA): "RGB2BGRA",          # :226-230
    (RGBA, GRAY): "RGBA2GRAY", (RGBA, BGR): "RGBA2BGR", (RGBA, RGB): "RGBA2RGB", (RGBA, BGRA): "RGBA2BGRA",                         # :239-242
    (RGBA, YUV): "RGBA2RGB, RGB2YUV",                                                                                                  # :245-249
    (YUV, GRAY): "extractChannel 0", (YUV, BGR): "YUV2BGR", (YUV, BGRA): "YUV2BGR dcn 4", (YUV, RGB): "YUV2RGB",                     # :260-263
    (YUV, RGBA): "YUV2RGB dcn 4",                                                                                                      # :264
    (GRAY, RGB): "GRAY2RGB", (GRAY, BGR): "GRAY2BGR", (GRAY, RGBA): "GRAY2RGBA", (GRAY, BGRA): "GRAY2BGRA",                         # :274-277
    (GRAY, YUV): "merge(gray, 128, 128)",                                                                                              # :278-294
}


def reformat(img, src, dst):
    """VideoFrame::reformatTo of a packed uint8 frame [rows, cols, C] (GRAY may also be [rows, cols]); returns [rows, cols, C']."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = img[..., None]
    assert img.shape[-1] == CHANNELS[src], (img.shape, src)
    if src == dst:
        return img.copy()
    assert (src, dst) in PAIRS, (src, dst)
    if src in (BGR, BGRA, RGB, RGBA):
        b, g, r = _bgr_planes(img, src)
        if dst == GRAY:
            return _sat(gray_of(b, g, r))[..., None]
        if dst == YUV:
            # BGRA / RGBA go through their 3-channel frame (VideoFrame.cpp:214-215,247-248): the alpha drops out either way
            return _sat(np.stack(yuv_of(b, g, r), axis=-1))
        # RGB2RGB<uchar>: 4 -> 4 keeps the source's alpha, 3 -> 4 writes 255
        return _pack(dst, b, g, r, img[..., 3].astype(np.int32) if CHANNELS[src] == 4 else None)
    if src == YUV:
        if dst == GRAY:
            return img[..., :1].copy()
        x = img.astype(np.int32)
        return _pack(dst, *bgr_of_yuv(x[..., 0], x[..., 1], x[..., 2]))
    # GRAY
    g = img[..., 0].astype(np.int32)
    if dst == YUV:
        return _sat(np.stack([g, np.full_like(g, 128), np.full_like(g, 128)], axis=-1))
    return _pack(dst, g, g, g)


def convert(img, src_fmt, code, dcn=0):
    """ConversionFilter: cvtColor(code, dcn) of a src_fmt frame; returns (frame, destination format)."""
    dst = code_target(code, src_fmt, dcn)
    assert dst >= 0, (code, src_fmt, dcn)
    return reformat(img, src_fmt, dst), dst
