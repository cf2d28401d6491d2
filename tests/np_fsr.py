"""Independent numpy restatement of the OBS plugin's FSR filter: FSRFilter::tick / FSREffect on the host, the FidelityFX FSR 1 EASU pass
(FsrEasuCon on the CPU, FsrEasuF / FsrEasuSetF / FsrEasuTapF) with fsr.effect's point-sampled gather on the pixels.  RCAS is not part of
it: the plugin runs EASU only and leaves sharpening to the CAS filter (np_cas).

Every operation is float32 and rounded on its own (no fused multiply-adds); the approximate reciprocals and inverse square root are the
FidelityFX bit tricks on the float's uint32 pattern.  Names: the viewport is the crop region (rx, ry, rw, rh) of a W x H frame, and the
output is ow x oh.

  host      con0 = (rw rcp(ow), rh rcp(oh), (0.5 rw) rcp(ow) - 0.5, (0.5 rh) rcp(oh) - 0.5),  con1 = (rcp(W), rcp(H), rcp(W), -rcp(H)),
            con2 = (-rcp(W), 2 rcp(H), rcp(W), 2 rcp(H)),  con3 = (0, 4 rcp(H), 0, 0);  per launch region_uv_offset = (rx / W, ry / H) and
            half = (0.5 / W, 0.5 / H)
  position  pp = ip con0.xy + con0.zw for the output pixel ip = (x, y), fp = floor(pp), pp -= fp
  gathers   p0 = fp con1.xy + con1.zw, p1 = p0 + con2.xy, p2 = p0 + con2.zw, p3 = p0 + con3.xy; each gather adds region_uv_offset and
            point-samples (p.x - h.x, p.y + h.y), (p.x + h.x, p.y + h.y), (p.x + h.x, p.y - h.y), (p.x - h.x, p.y - h.y), texel
            clamp(floor(u W), 0, W - 1) x clamp(floor(v H), 0, H - 1): the clamp is to the frame, not the region
  luma      0.5 b + (0.5 r + g)
  direction four bilinear FsrEasuSetF accumulations, dirR < 1/32768 guard, lo_rsq, stretch, len2, lob, clp = lo_rcp(lob)
  taps      12 weighted taps in the order b c i j f e k l h g o n, normalised by a correctly rounded 1 / aW, clamped to min / max of f g j k
  load      x = u8 / 255, correctly rounded (as np_cas)
  store     rint(pix 255), round half to even; a 4th channel is written as 255 (the shader returns float4(col, 1.0))

Declared choices:
  1. All arithmetic is unfused float32, each operation rounded on its own.
  2. rcp, rx / W and 0.5 / W are correctly rounded: OBS on OpenGL, where ARcpF1 is 1 / x, and FsrEasuCon's CPU path.
  3. r, g, b are the frame's red, green and blue bytes for BGR / BGRA / RGB / RGBA; for YUV they are bytes 0, 1, 2.
  4. The stored bytes are filtered as they are (OBS's linear-sRGB mode off).
  5. The output size comes from the current frame's size (the plugin uses the previous render's).
  6. The texel choice of the point sampler is not a choice: every sampled u W lies at k + 0.5 +- a tiny error (`sample_coords`), so
     the texel is (fp.x + rx + {-1, 0, 1, 2}, fp.y + ry + {-1, 0, 1, 2}) clamped to the frame, whatever the rounding of u W.

The float64 `textbook_easu` (exact reciprocal and square root, no float32 rounding) is a bound for the restatement, not a specification.
"""
import numpy as np

from tests.np_cas import UNIT, _as_f32, _as_u32, lo_rcp, sat

f32 = np.float32
u32 = np.uint32
FMT_BGR, FMT_BGRA, FMT_RGB, FMT_RGBA, FMT_YUV, FMT_GRAY = 0, 1, 2, 3, 4, 5
CHANNELS = {FMT_BGR: 3, FMT_RGB: 3, FMT_YUV: 3, FMT_BGRA: 4, FMT_RGBA: 4}
MAX_DIMENSION = 4096                                   # FSRFilter.cpp: OUTPUT_MAX_DIMENSION, also the crop limit

# float32 roundings of the double literals of FsrEasuTapF / FsrEasuF
W_B = f32(2.0 / 5.0)
W_SCALE = f32(25.0 / 16.0)
W_BIAS = f32(-(25.0 / 16.0 - 1.0))
LOB_SLOPE = f32((1.0 / 4.0 - 0.04) - 0.5)
DIR_EPS = f32(1.0 / 32768.0)


def lo_rsq(v):
    """APrxLoRsqF1: as_float(0x5f347d74 - (as_uint(v) >> 1))."""
    return _as_f32(u32(0x5f347d74) - (_as_u32(v) >> u32(1)))


def rcp(v):
    """ARcpF1 on OpenGL and the CPU: 1 / v, correctly rounded."""
    return f32(1) / np.asarray(v, dtype=f32)


def easu_const(rw, rh, W, H, ow, oh):
    """FsrEasuCon(con0..con3, viewport rw x rh, input W x H, output ow x oh) on the CPU: 16 float32 values."""
    rw, rh, W, H, ow, oh = (f32(v) for v in (rw, rh, W, H, ow, oh))
    con = np.zeros(16, f32)
    con[0] = rw * rcp(ow)
    con[1] = rh * rcp(oh)
    con[2] = (f32(0.5) * rw) * rcp(ow) - f32(0.5)
    con[3] = (f32(0.5) * rh) * rcp(oh) - f32(0.5)
    con[4], con[5], con[6], con[7] = rcp(W), rcp(H), f32(1) * rcp(W), f32(-1) * rcp(H)
    con[8], con[9], con[10], con[11] = f32(-1) * rcp(W), f32(2) * rcp(H), f32(1) * rcp(W), f32(2) * rcp(H)
    con[12], con[13] = f32(0) * rcp(W), f32(4) * rcp(H)
    return con


# ---- output geometry: FSRFilter::tick + FSREffect::should_skip + OBSEffect::is_renderable -------------------------------------------

def cv_round(v):
    """cvRound of a float32 (cv::Size2f assigned to cv::Size): round half to even."""
    return int(np.rint(f32(v)))


def geometry(rows, cols, out_size=None, multiplier=1.0, maintain_aspect_ratio=True, crop=(0, 0, 0, 0)):
    """(region (x, y, w, h), output (rows, cols), skip) for a rows x cols frame.  out_size = (rows, cols) of an explicit output, or None
    for source x multiplier; crop = (left, top, right, bottom)."""
    if out_size is None:
        m = f32(multiplier)
        ow, oh = cv_round(f32(cols) * m), cv_round(f32(rows) * m)
    else:
        oh, ow = out_size
    l, t, r, b = crop
    if l + r < cols and t + b < rows:
        region = (l, t, cols - r - l, rows - b - t)
    else:
        region = (0, 0, cols, rows)
    rw, rh = region[2], region[3]
    if maintain_aspect_ratio and rw * rh != 0:
        s = min(f32(ow) / f32(rw), f32(oh) / f32(rh))
        ow, oh = cv_round(f32(rw) * s), cv_round(f32(rh) * s)
    ow, oh = min(ow, MAX_DIMENSION), min(oh, MAX_DIMENSION)
    skip = ow <= 0 or oh <= 0 or ((ow, oh) == (cols, rows) and (rw, rh) == (cols, rows))
    return region, (oh, ow), skip


# ---- EASU ---------------------------------------------------------------------------------------------------------------------------

# (dx, dy) of each tap relative to 'f' = (fp.x, fp.y), and which gather (p0..p3) and which of its x y z w holds it
TAPS = {"b": (0, -1), "c": (1, -1), "e": (-1, 0), "f": (0, 0), "g": (1, 0), "h": (2, 0),
        "i": (-1, 1), "j": (0, 1), "k": (1, 1), "l": (2, 1), "n": (0, 2), "o": (1, 2)}
GATHERS = [("b", "c", None, None), ("i", "j", "f", "e"), ("k", "l", "h", "g"), (None, None, "o", "n")]
ORDER = "bcijfeklhgon"


def _positions(rows, cols, region, out_rows, out_cols):
    """pp fractions and, per gather, the scaled sample coordinates (u W, v H) of its x y z w: float32 arrays over output columns / rows."""
    rx, ry, rw, rh = region
    con = easu_const(rw, rh, cols, rows, out_cols, out_rows)
    W, H = f32(cols), f32(rows)
    off = (f32(rx) / W, f32(ry) / H)
    half = (f32(0.5) / W, f32(0.5) / H)
    out = {}
    for axis, n in ((0, out_cols), (1, out_rows)):
        ip = np.arange(n, dtype=f32)
        pp = ip * con[axis] + con[2 + axis]
        fp = np.floor(pp)
        pp = pp - fp
        p0 = fp * con[4 + axis] + con[6 + axis]
        ps = [p0, p0 + con[8 + axis], p0 + con[10 + axis], p0 + con[12 + axis]]
        size = (W, H)[axis]
        coords = []
        for p in ps:
            p = p + off[axis]
            # x y z w: x at (-h, +h), y at (+h, +h), z at (+h, -h), w at (-h, -h)
            signs = (-1, 1, 1, -1) if axis == 0 else (1, 1, -1, -1)
            coords.append([(p - half[axis] if s < 0 else p + half[axis]) * size for s in signs])
        out[axis] = (pp, fp, coords)
    return out


def sample_coords(rows, cols, region, out_rows, out_cols):
    """Every scaled sample coordinate u W (and v H) the shader's point sampler sees, with the texel index the float formula picks and the
    one the integer formula picks (fp + r + d, d in -1..2).  For declared choice 6."""
    pos = _positions(rows, cols, region, out_rows, out_cols)
    res = []
    for axis in (0, 1):
        pp, fp, coords = pos[axis]
        r = region[axis]
        for gi, names in enumerate(GATHERS):
            for q, name in enumerate(names):
                if name is None:
                    continue
                d = TAPS[name][axis]
                res.append((coords[gi][q], np.floor(coords[gi][q]), fp + f32(r + d)))
    return res


def _texel_index(scaled, size):
    return np.clip(np.floor(scaled), 0, size - 1).astype(np.int64)


def channel_bytes(fmt):
    """Byte indices of the shader's r, g, b in a pixel of the format (declared choice 3)."""
    return (2, 1, 0) if fmt in (FMT_BGR, FMT_BGRA) else (0, 1, 2)


def luma(tr, tg, tb):
    """Twice an approximate luma: 0.5 b + (0.5 r + g)."""
    return tb * f32(0.5) + (tr * f32(0.5) + tg)


def easu_unit(r, g, b, region, out_rows, out_cols, row_block=256):
    """FsrEasuF on float32 [H, W] planes r, g, b of values in [0, 1]; returns the float32 [out_rows, out_cols, 3] (r, g, b) result."""
    rows, cols = r.shape
    pos = _positions(rows, cols, region, out_rows, out_cols)
    ppx, _, cx = pos[0]
    ppy_all, _, cy_all = pos[1]
    col_idx = {}
    for gi, names in enumerate(GATHERS):
        for q, name in enumerate(names):
            if name is not None:
                col_idx[name] = _texel_index(cx[gi][q], cols)
    out = np.empty((out_rows, out_cols, 3), f32)
    for y0 in range(0, out_rows, row_block):
        y1 = min(y0 + row_block, out_rows)
        ppy = ppy_all[y0:y1, None]
        px = ppx[None, :]
        taps = {}
        for gi, names in enumerate(GATHERS):
            for q, name in enumerate(names):
                if name is None:
                    continue
                ri = _texel_index(cy_all[gi][q][y0:y1], rows)[:, None]
                ci = col_idx[name][None, :]
                tr, tg, tb = r[ri, ci], g[ri, ci], b[ri, ci]
                taps[name] = (tr, tg, tb, luma(tr, tg, tb))
        out[y0:y1] = _easu_core(taps, px, ppy)
    return out


def _easu_core(taps, ppx, ppy):
    L = {k: v[3] for k, v in taps.items()}
    one = f32(1)
    dirx = f32(0)
    diry = f32(0)
    ln = f32(0)

    def set_f(w, lA, lB, lC, lD, lE):
        nonlocal dirx, diry, ln
        dc = lD - lC
        cb = lC - lB
        lenx = lo_rcp(np.maximum(np.abs(dc), np.abs(cb)))
        dx = lD - lB
        dirx = dirx + dx * w
        lenx = sat(np.abs(dx) * lenx)
        lenx = lenx * lenx
        ln = ln + lenx * w
        ec = lE - lC
        ca = lC - lA
        leny = lo_rcp(np.maximum(np.abs(ec), np.abs(ca)))
        dy = lE - lA
        diry = diry + dy * w
        leny = sat(np.abs(dy) * leny)
        leny = leny * leny
        ln = ln + leny * w

    with np.errstate(over="ignore", invalid="ignore"):
        set_f((one - ppx) * (one - ppy), L["b"], L["e"], L["f"], L["g"], L["j"])
        set_f(ppx * (one - ppy), L["c"], L["f"], L["g"], L["h"], L["k"])
        set_f((one - ppx) * ppy, L["f"], L["i"], L["j"], L["k"], L["n"])
        set_f(ppx * ppy, L["g"], L["j"], L["k"], L["l"], L["o"])
    dir2x = dirx * dirx
    dir2y = diry * diry
    dirr = dir2x + dir2y
    zro = dirr < DIR_EPS
    dirr = np.where(zro, one, lo_rsq(dirr))
    dirx = np.where(zro, one, dirx)
    dirx = dirx * dirr
    diry = diry * dirr
    ln = ln * f32(0.5)
    ln = ln * ln
    stretch = (dirx * dirx + diry * diry) * lo_rcp(np.maximum(np.abs(dirx), np.abs(diry)))
    len2x = one + (stretch - one) * ln
    len2y = one + f32(-0.5) * ln
    lob = f32(0.5) + LOB_SLOPE * ln
    clp = lo_rcp(lob)

    ac = [f32(0)] * 3
    aw = f32(0)
    for name in ORDER:
        ox, oy = TAPS[name]
        offx = f32(ox) - ppx
        offy = f32(oy) - ppy
        vx = (offx * dirx) + (offy * diry)
        vy = (offx * (-diry)) + (offy * dirx)
        vx = vx * len2x
        vy = vy * len2y
        d2 = vx * vx + vy * vy
        d2 = np.minimum(d2, clp)
        wb = W_B * d2 + f32(-1)
        wa = lob * d2 + f32(-1)
        wb = wb * wb
        wa = wa * wa
        wb = W_SCALE * wb + W_BIAS
        w = wb * wa
        ac = [ac[c] + taps[name][c] * w for c in range(3)]
        aw = aw + w
    inv = rcp(aw)
    res = []
    for c in range(3):
        mn = np.fmin(np.fmin(np.fmin(taps["f"][c], taps["g"][c]), taps["j"][c]), taps["k"][c])
        mx = np.fmax(np.fmax(np.fmax(taps["f"][c], taps["g"][c]), taps["j"][c]), taps["k"][c])
        res.append(np.fmin(mx, np.fmax(mn, ac[c] * inv)))
    return np.stack(res, -1)


def fsr(img, fmt, region, out_rows, out_cols):
    """The EASU pass on a uint8 [rows, cols, 3 | 4] frame of format fmt: the region (x, y, w, h) scaled to out_rows x out_cols."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == CHANNELS[fmt]
    ri, gi, bi = channel_bytes(fmt)
    x = UNIT[img]
    y = easu_unit(x[..., ri], x[..., gi], x[..., bi], region, out_rows, out_cols)
    out = np.empty((out_rows, out_cols, img.shape[2]), np.uint8)
    q = np.rint(y * f32(255)).astype(np.uint8)
    out[..., ri], out[..., gi], out[..., bi] = q[..., 0], q[..., 1], q[..., 2]
    if img.shape[2] == 4:
        out[..., 3] = 255
    return out


def fsr_filter(img, fmt, out_size=None, multiplier=1.0, maintain_aspect_ratio=True, crop=(0, 0, 0, 0)):
    """FSRFilter on one frame: the geometry, then EASU, or the frame itself when the geometry skips."""
    region, (oh, ow), skip = geometry(img.shape[0], img.shape[1], out_size, multiplier, maintain_aspect_ratio, crop)
    return np.array(img, copy=True) if skip else fsr(img, fmt, region, oh, ow)


def textbook_easu(img, fmt, region, out_rows, out_cols):
    """A float64 EASU: the same taps and shape, with exact reciprocals and square roots and no float32 rounding (the tests' bound)."""
    img = np.asarray(img)
    rows, cols = img.shape[:2]
    rx, ry, rw, rh = region
    ri, gi, bi = channel_bytes(fmt)
    x = img.astype(np.float64) / 255.0
    sx, sy = rw / out_cols, rh / out_rows
    ppx = np.arange(out_cols) * sx + (0.5 * sx - 0.5)
    ppy = (np.arange(out_rows) * sy + (0.5 * sy - 0.5))[:, None]
    fpx, fpy = np.floor(ppx), np.floor(ppy)
    ppx, ppy = ppx - fpx, ppy - fpy
    taps = {}
    for name, (dx, dy) in TAPS.items():
        ci = np.clip(fpx.astype(np.int64) + rx + dx, 0, cols - 1)[None, :]
        rj = np.clip(fpy.astype(np.int64) + ry + dy, 0, rows - 1)
        tr, tg, tb = x[rj, ci, ri], x[rj, ci, gi], x[rj, ci, bi]
        taps[name] = (tr, tg, tb, 0.5 * tb + 0.5 * tr + tg)
    L = {k: v[3] for k, v in taps.items()}
    dirx = diry = ln = 0.0
    for w, (lA, lB, lC, lD, lE) in (((1 - ppx) * (1 - ppy), "befgj"), (ppx * (1 - ppy), "cfghk"), ((1 - ppx) * ppy, "fijkn"), (ppx * ppy, "gjklo")):
        a, b_, c, d, e = L[lA], L[lB], L[lC], L[lD], L[lE]
        with np.errstate(divide="ignore", invalid="ignore"):
            lx = np.where(np.maximum(abs(d - c), abs(c - b_)) > 0, np.clip(abs(d - b_) / np.maximum(abs(d - c), abs(c - b_)), 0, 1), 0.0)
            ly = np.where(np.maximum(abs(e - c), abs(c - a)) > 0, np.clip(abs(e - a) / np.maximum(abs(e - c), abs(c - a)), 0, 1), 0.0)
        dirx = dirx + (d - b_) * w
        diry = diry + (e - a) * w
        ln = ln + (lx * lx + ly * ly) * w
    dr = dirx * dirx + diry * diry
    zro = dr < 1.0 / 32768.0
    with np.errstate(divide="ignore"):
        inv = np.where(zro, 1.0, 1.0 / np.sqrt(np.where(zro, 1.0, dr)))
    dirx = np.where(zro, 1.0, dirx) * inv
    diry = diry * inv
    ln = (ln * 0.5) ** 2
    stretch = (dirx * dirx + diry * diry) / np.maximum(abs(dirx), abs(diry))
    len2x, len2y = 1 + (stretch - 1) * ln, 1 - 0.5 * ln
    lob = 0.5 + ((0.25 - 0.04) - 0.5) * ln
    clp = 1.0 / lob
    ac, aw = [0.0, 0.0, 0.0], 0.0
    for name in ORDER:
        ox, oy = TAPS[name]
        offx, offy = ox - ppx, oy - ppy
        vx = (offx * dirx + offy * diry) * len2x
        vy = (-offx * diry + offy * dirx) * len2y
        d2 = np.minimum(vx * vx + vy * vy, clp)
        w = (25 / 16 * (0.4 * d2 - 1) ** 2 - (25 / 16 - 1)) * (lob * d2 - 1) ** 2
        ac = [ac[c] + taps[name][c] * w for c in range(3)]
        aw = aw + w
    out = np.empty((out_rows, out_cols, img.shape[2]), np.uint8)
    for c, bi_ in zip(range(3), (ri, gi, bi)):
        mn = np.minimum.reduce([taps[k][c] for k in "fgjk"])
        mx = np.maximum.reduce([taps[k][c] for k in "fgjk"])
        out[..., bi_] = np.rint(np.clip(ac[c] / aw, mn, mx) * 255).astype(np.uint8)
    if img.shape[2] == 4:
        out[..., 3] = 255
    return out
