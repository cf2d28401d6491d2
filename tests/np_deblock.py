"""Independent numpy restatement of lvk::DeblockingFilter (Filters/DeblockingFilter.cpp:48-138) under the OpenCV 4.8 CPU conventions of
DESIGN.md section 2 (the deblocking rows of section 13 list them).  Integer arithmetic where OpenCV's is integer, float32 (no fused
multiply-adds: every product and sum is its own numpy operation) where it is float, binary64 where the reference computes in double.

Operation order, as the reference runs it on the region of full macroblocks:
  1. small  = INTER_AREA(region, fx = fy = 1.f / s)            output size rint(n * (double)(1.f / s)), scale 1 / (double)(1.f / s)
  2. small  = medianBlur(small, k)                              exact per-channel median, BORDER_REPLICATE
  3. smooth = INTER_LINEAR(small -> region size), 8U            11-bit weights, vertical ((b * (S >> 4)) >> 16)
  4. gray   = reformatTo(GRAY); grid = INTER_AREA(gray -> extent); dev = |gray - grid[block]|; grid = INTER_AREA(dev -> extent)
  5. keep_block = float(min(grid, L) * (1.0 / L)) (binary64);  keep = INTER_LINEAR(keep_block -> region), float32;  deblock = |keep - 1|
  6. region = saturate_cast<uchar>((src * keep + smooth * deblock) / (keep + deblock + 1e-5f))
draw_influence repeats 6 with a constant MAGENTA[format] for `smooth` and the maps of the last apply.
"""
import numpy as np

f32 = np.float32
FMT_BGR, FMT_RGB, FMT_YUV = 0, 2, 4
MAGENTA = {FMT_BGR: (255, 0, 255), FMT_RGB: (255, 0, 255), FMT_YUV: (105, 212, 234)}      # lvk::col::MAGENTA[format]


def sat_u8(v):
    """cv::saturate_cast<uchar>(float): round half to even, then clamp."""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def gray_of(frame, fmt):
    """VideoFrame::reformatTo(GRAY): channel 0 of YUV, fixed-point BT.601 of BGR / RGB (OpenCV's RGB2Gray<uchar>)."""
    f = frame.astype(np.int32)
    if fmt == FMT_YUV:
        return f[..., 0]
    b, g, r = (f[..., 0], f[..., 1], f[..., 2]) if fmt == FMT_BGR else (f[..., 2], f[..., 1], f[..., 0])
    return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15


def small_size(n, s):
    """cv::resize(.., Size(), 1.f / s, 1.f / s): saturate_cast<int>(n * inv) with inv the float reciprocal promoted to double."""
    inv = float(f32(1) / f32(s))
    return int(np.rint(n * inv))


def area_tab(ssize, dsize, scale):
    """computeResizeAreaTab: per destination index the list of (source index, float32 weight)."""
    tab = [[] for _ in range(dsize)]
    for dx in range(dsize):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = int(np.ceil(fsx1)), int(np.floor(fsx2))
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        if sx1 - fsx1 > 1e-3:
            tab[dx].append((sx1 - 1, f32((sx1 - fsx1) / cell)))
        for sx in range(sx1, sx2):
            tab[dx].append((sx, f32(1.0 / cell)))
        if fsx2 - sx2 > 1e-3:
            tab[dx].append((sx2, f32(min(min(fsx2 - sx2, 1.0), cell) / cell)))
    return tab


def _tab_arrays(tab):
    n = max(len(t) for t in tab)
    idx = np.zeros((len(tab), n), np.int64)
    w = np.zeros((len(tab), n), f32)
    for d, t in enumerate(tab):
        for j, (i, a) in enumerate(t):
            idx[d, j], w[d, j] = i, a
    return idx, w


def area_resize(img, dh, dw, scale):
    """cv::resize(img, (dw, dh), INTER_AREA) with the hal's scale (both axes): img [H, W] or [H, W, C] uint8 / int."""
    img = np.asarray(img)
    squeeze = img.ndim == 2
    if squeeze:
        img = img[..., None]
    H, W = img.shape[:2]
    if (dh, dw) == (H, W):
        out = img.astype(np.uint8)
    else:
        iscale = int(np.rint(scale))
        if abs(scale - iscale) < 2.220446049250313e-16:
            out = _area_fast(img.astype(np.int64), dh, dw, iscale)
        else:
            out = _area_generic(img, dh, dw, scale)
    return out[..., 0] if squeeze else out


def _area_fast(img, dh, dw, k):
    """resizeAreaFast_: integer box sum * (1.f / area) rounded half to even; 2 x 2 as (sum + 2) >> 2.  Cells that reach past the source
    (a destination size rounded up) average what they cover: (float)sum / count."""
    H, W, C = img.shape
    out = np.empty((dh, dw, C), np.uint8)
    fh, fw = min(dh, H // k), min(dw, W // k)
    if fh and fw:
        s = img[:fh * k, :fw * k].reshape(fh, k, fw, k, C).sum(axis=(1, 3))
        if k == 2:
            out[:fh, :fw] = ((s + 2) >> 2).astype(np.uint8)
        else:
            out[:fh, :fw] = sat_u8(s.astype(f32) * (f32(1) / f32(k * k)))
    for y in range(dh):
        for x in range(dw):
            if y < fh and x < fw:
                continue
            cell = img[y * k:min(y * k + k, H), x * k:min(x * k + k, W)]
            cnt = cell.shape[0] * cell.shape[1]
            out[y, x] = sat_u8(cell.sum(axis=(0, 1)).astype(f32) / f32(cnt))
    return out


def _area_generic(img, dh, dw, scale):
    """resizeArea_: separable tables, float32 accumulation in table order (per row taps along x, then the rows weighted by beta)."""
    H, W, C = img.shape
    xi, xw = _tab_arrays(area_tab(W, dw, scale))
    yi, yw = _tab_arrays(area_tab(H, dh, scale))
    src = img.astype(f32)
    buf = np.zeros((H, dw, C), f32)
    for j in range(xi.shape[1]):
        buf = buf + src[:, xi[:, j]] * xw[:, j][None, :, None]
    acc = np.zeros((dh, dw, C), f32)
    for j in range(yi.shape[1]):
        acc = acc + yw[:, j][:, None, None] * buf[yi[:, j]]
    return sat_u8(acc)


def median(img, k):
    """medianBlur(img, k): per-channel median of the k x k window, BORDER_REPLICATE."""
    r = k // 2
    p = np.pad(img, ((r, r), (r, r), (0, 0)), mode="edge")
    win = np.lib.stride_tricks.sliding_window_view(p, (k, k), axis=(0, 1))
    win = win.reshape(img.shape + (k * k,))
    return np.partition(win, k * k // 2, axis=-1)[..., k * k // 2].astype(np.uint8)


def lin_tab(ssize, dsize, vertical):
    """cv::resize INTER_LINEAR coordinates (scale = ssize / dsize): (s0, s1, fraction); columns clamp with a single tap past the end."""
    scale = 1.0 / (dsize / ssize)
    s0 = np.empty(dsize, np.int64); s1 = np.empty(dsize, np.int64); fr = np.empty(dsize, f32); single = np.zeros(dsize, bool)
    for d in range(dsize):
        fx = f32((d + 0.5) * scale - 0.5)
        s = int(np.floor(fx))
        fx = f32(fx - f32(s))
        if vertical:
            s0[d], s1[d], fr[d] = min(max(s, 0), ssize - 1), min(max(s + 1, 0), ssize - 1), fx
            continue
        if s < 0:
            fx, s = f32(0), 0
        if s + 1 >= ssize:
            single[d] = True
            if s >= ssize - 1:
                fx, s = f32(0), ssize - 1
        s0[d], s1[d], fr[d] = s, (s if single[d] else s + 1), fx
    return s0, s1, fr, single


def resize_linear_u8(img, dh, dw):
    """cv::resize(8UC3, INTER_LINEAR): 11-bit coefficients, HResizeLinear in int, VResizeLinear ((b * (S >> 4)) >> 16 ... + 2) >> 2."""
    H, W = img.shape[:2]
    xs0, xs1, xf, xsingle = lin_tab(W, dw, False)
    ys0, ys1, yf, _ = lin_tab(H, dh, True)
    a0 = np.where(xsingle, 2048, np.rint((f32(1) - xf) * f32(2048))).astype(np.int64)
    a1 = np.where(xsingle, 0, np.rint(xf * f32(2048))).astype(np.int64)
    b0 = np.rint((f32(1) - yf) * f32(2048)).astype(np.int64)
    b1 = np.rint(yf * f32(2048)).astype(np.int64)
    S = img.astype(np.int64)
    h = S[:, xs0] * a0[None, :, None] + S[:, xs1] * a1[None, :, None]
    v = ((b0[:, None, None] * (h[ys0] >> 4)) >> 16) + ((b1[:, None, None] * (h[ys1] >> 4)) >> 16)
    return ((v + 2) >> 2).astype(np.uint8)


def resize_linear_f32(img, dh, dw):
    """cv::resize(32FC1, INTER_LINEAR): S[s0] * a0 + S[s1] * a1 along x (tail: a0 = 1, a1 = 0), then H0 * b0 + H1 * b1; no fusion."""
    H, W = img.shape
    xs0, xs1, xf, xsingle = lin_tab(W, dw, False)
    ys0, ys1, yf, _ = lin_tab(H, dh, True)
    a0 = np.where(xsingle, f32(1), f32(1) - xf).astype(f32)
    a1 = np.where(xsingle, f32(0), xf).astype(f32)
    b0 = (f32(1) - yf).astype(f32)
    b1 = yf
    S = img.astype(f32)
    h = S[:, xs0] * a0[None, :] + S[:, xs1] * a1[None, :]
    return h[ys0] * b0[:, None] + h[ys1] * b1[:, None]


def block_grid(gray, bs):
    """INTER_AREA of a region of whole bs x bs blocks to one value per block (integer scale bs)."""
    ey, ex = gray.shape[0] // bs, gray.shape[1] // bs
    return area_resize(gray, ey, ex, float(bs)).astype(np.int32)


def keep_block_of(grid, levels):
    """The threshold loop of DeblockingFilter.cpp:86-95: keep = (l + 1.0) * (1.0 / L) for the largest l < grid, in binary64, stored as float."""
    return (np.minimum(grid, levels).astype(np.float64) * (1.0 / levels)).astype(f32)


def blend(src, other, keep):
    """cv::blendLinear(src, other, keep, |keep - 1|): (src * w1 + other * w2) / (w1 + w2 + 1e-5f) per channel, float32."""
    deb = np.abs(keep - f32(1))
    w1, w2 = keep[..., None], deb[..., None]
    num = src.astype(f32) * w1 + np.asarray(other).astype(f32) * w2
    den = (w1 + w2) + f32(1e-5)
    return sat_u8(num / den)


def deblock(frame, fmt, detection_levels=3, block_size=16, filter_size=5, filter_scaling=4.0):
    """DeblockingFilter::filter on a copy of `frame` ([rows, cols, 3] uint8).  Returns (out, info); info carries the region (x, y, w, h),
    the intermediate images and the keep map draw_influence reuses.  Raises ValueError where the library refuses the frame."""
    bs, L, k, s = int(block_size), int(detection_levels), int(filter_size), float(filter_scaling)
    rows, cols = frame.shape[:2]
    ey, ex = rows // bs, cols // bs
    RH, RW = ey * bs, ex * bs
    if ey == 0 or ex == 0:
        raise ValueError("no whole macroblock")
    hs, ws = small_size(RH, s), small_size(RW, s)
    if hs <= 0 or ws <= 0:
        raise ValueError("empty downscale")
    region = frame[:RH, :RW]
    scale = 1.0 / float(f32(1) / f32(s))
    small = area_resize(region, hs, ws, scale)
    med = median(small, k)
    smooth = resize_linear_u8(med, RH, RW)
    gray = gray_of(region, fmt)
    mean = block_grid(gray, bs)
    dev = np.abs(gray - np.repeat(np.repeat(mean, bs, axis=0), bs, axis=1))
    grid = block_grid(dev, bs)
    kb = keep_block_of(grid, L)
    keep = resize_linear_f32(kb, RH, RW)
    out = frame.copy()
    out[:RH, :RW] = blend(region, smooth, keep)
    info = dict(region=(0, 0, RW, RH), small=small, median=med, smooth=smooth, mean=mean.astype(np.uint8), grid=grid.astype(np.uint8),
                keep_block=kb, keep=keep)
    return out, info


def draw_influence(frame, fmt, info):
    """DeblockingFilter::draw_influence: blends MAGENTA[format] into the last region with the last keep map (on a copy)."""
    _, _, RW, RH = info["region"]
    out = frame.copy()
    out[:RH, :RW] = blend(frame[:RH, :RW], np.array(MAGENTA[fmt], np.uint8)[None, None, :], info["keep"])
    return out
