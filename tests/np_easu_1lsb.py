"""Specification of the opt-in remap precision LVK_REMAP_1LSB (include/lvk_hip.h), in vectorised numpy (float32) on top of
tests/np_easu.py's helpers.

The mode is the EASU remap of np_easu.py -- same 12 taps, same direction analysis on the normalised colours, same min / max clamp and x 255 truncation --
with ONE stage restated: the twelve window weights.  Where FSR.cl:98-126 rotates, scales and squares each tap's offset and evaluates the window as
(25/16 (2/5 d2 - 1)^2 - 9/16) (lob d2 - 1)^2, this form uses the algebra of the same expressions:

  * d2 = |diag(len2) R(dir) off|^2 is a quadratic form in off = (ox, oy):  d2 = (q11 ox + 2 q12 oy) ox + q22 oy^2  with
    a = len2x dirx, b = len2x diry, c = len2y diry, d = len2y dirx,  q11 = a^2 + c^2,  q22 = b^2 + d^2,  q12 = a b - c d;
  * the window is  ((u / 4 - 5 / 4) u + 1) (lob u - 1)^2  with u = min(d2, clp);
  * the taps are accumulated in row order  b c e f g h i j k l n o.

The results differ from the reference's operation sequence by float32 rounding only: every output byte is within 1 of np_easu's, and almost all are equal
(tests/test_remap_precision_spec.py).  The kernels are remap_core.hpp's EasuRegrouped weight stage.
"""
import numpy as np

from tests.np_easu import _fma, _rcp_lo, _rsq_lo, _sat, f32


def easu_points(src, sx, sy, ppx, ppy, yuv):
    """np_easu.easu_points with the regrouped weight stage.  src [rows, cols, 3] uint8; sx, sy int arrays (valid EASU interior); ppx, ppy float32 arrays."""
    norm = f32(0.00392156862)

    def px(dx, dy):
        return src[sy + dy, sx + dx].astype(f32) * norm

    b, c = px(0, -1), px(1, -1)
    e, f, g, h = px(-1, 0), px(0, 0), px(1, 0), px(2, 0)
    i, j, k, l = px(-1, 1), px(0, 1), px(1, 1), px(2, 1)
    n, o = px(0, 2), px(1, 2)

    def luma(p):
        if yuv:
            return _fma(p[..., 2], f32(0.5), _fma(p[..., 0], f32(0.5), p[..., 1]))
        return p[..., 0]

    L = {name: luma(v) for name, v in dict(b=b, c=c, e=e, f=f, g=g, h=h, i=i, j=j, k=k, l=l, n=n, o=o).items()}
    one = f32(1)
    dirx = np.zeros_like(ppx); diry = np.zeros_like(ppx); ln = np.zeros_like(ppx)

    # ---- the direction analysis: np_easu.py's sequence, unchanged (FSR.cl:131-176,244-277)
    def acc(w, lA, lB, lC, lD, lE):
        nonlocal dirx, diry, ln
        dc = lD - lC; cb = lC - lB
        lenX = _rcp_lo(np.maximum(np.abs(dc), np.abs(cb)))
        dX = lD - lB
        dirx = _fma(dX, w, dirx)
        lenX = _sat(np.abs(dX) * lenX); lenX = lenX * lenX
        ln = _fma(lenX, w, ln)
        ec = lE - lC; ca = lC - lA
        lenY = _rcp_lo(np.maximum(np.abs(ec), np.abs(ca)))
        dY = lE - lA
        diry = _fma(dY, w, diry)
        lenY = _sat(np.abs(dY) * lenY); lenY = lenY * lenY
        ln = _fma(lenY, w, ln)

    omx, omy = one - ppx, one - ppy
    acc(omx * omy, L['b'], L['e'], L['f'], L['g'], L['j'])
    acc(ppx * omy, L['c'], L['f'], L['g'], L['h'], L['k'])
    acc(omx * ppy, L['f'], L['i'], L['j'], L['k'], L['n'])
    acc(ppx * ppy, L['g'], L['j'], L['k'], L['l'], L['o'])

    dirR = dirx * dirx + diry * diry
    zro = dirR < f32(1.0 / 32768.0)
    dirR = _rsq_lo(dirR)
    dirR = np.where(zro, one, dirR)
    dirx = np.where(zro, one, dirx)
    dirx = dirx * dirR; diry = diry * dirR
    ln = ln * f32(0.5); ln = ln * ln
    stretch = _fma(dirx, dirx, diry * diry) * _rcp_lo(np.maximum(np.abs(dirx), np.abs(diry)))
    len2x = _fma(stretch - one, ln, one)
    len2y = _fma(f32(-0.5), ln, one)
    lob = _fma((f32(1.0) / f32(4.0) - f32(0.04)) - f32(0.5), ln, f32(0.5))
    clp = _rcp_lo(lob)

    mi4 = np.minimum(np.minimum(f, g), np.minimum(j, k))
    ma4 = np.maximum(np.maximum(f, g), np.maximum(j, k))

    # ---- the weight stage, regrouped
    qa = len2x * dirx; qb = len2x * diry; qc = len2y * diry; qd = len2y * dirx      # rows of diag(len2) R(dir): (a, b), (-c, d)
    q11 = _fma(qa, qa, qc * qc); q22 = _fma(qb, qb, qd * qd)
    q12 = _fma(qa, qb, -(qc * qd))
    q12x2 = q12 + q12
    aC = np.zeros(ppx.shape + (3,), f32); aW = np.zeros_like(ppx)

    def row(oy_int, taps):
        nonlocal aC, aW
        oy = f32(oy_int) - ppy
        E = q12x2 * oy
        B = (q22 * oy) * oy
        for ox_int, col in taps:
            ox = f32(ox_int) - ppx
            u = np.minimum(_fma(_fma(q11, ox, E), ox, B), clp)
            sA = _fma(lob, u, f32(-1))
            qB = _fma(_fma(u, f32(0.25), f32(-1.25)), u, one)
            w = qB * (sA * sA)
            aC = _fma(col, w[..., None], aC)
            aW = aW + w

    row(-1, ((0, b), (1, c)))
    row(0, ((-1, e), (0, f), (1, g), (2, h)))
    row(1, ((-1, i), (0, j), (1, k), (2, l)))
    row(2, ((0, n), (1, o)))

    # ---- normalise, clamp, truncate: np_easu.py's sequence, unchanged (FSR.cl:316-317)
    rW = one / aW
    fpx = np.minimum(ma4, np.maximum(mi4, aC * rW[..., None]))
    return (fpx * f32(255.0)).astype(np.int32).astype(np.uint8)


def remap_tail(src, subx, suby, bg, yuv):
    """np_easu._remap_tail with the regrouped core.  Also returns the mask of the pixels that reach the weights (all others -- the border band's nearest
    copies and the background -- are np_easu's bytes by construction)."""
    rows, cols = src.shape[:2]
    sx = np.trunc(np.clip(subx, -2e9, 2e9)).astype(np.int64)
    sy = np.trunc(np.clip(suby, -2e9, 2e9)).astype(np.int64)
    ppx = subx - np.floor(subx); ppy = suby - np.floor(suby)
    out = np.empty(src.shape, np.uint8)
    out[...] = np.asarray(bg, np.uint8)
    border = (sx < 1) | (sy < 1) | (sx >= cols - 4) | (sy >= rows - 4)
    inside = (sx >= 0) & (sx < cols) & (sy >= 0) & (sy < rows)
    nn = border & inside
    out[nn] = src[sy[nn], sx[nn]]
    ea = ~border
    if ea.any():
        out[ea] = easu_points(src, sx[ea], sy[ea], ppx[ea].astype(f32), ppy[ea].astype(f32), yuv)
    return out, ea


def homography_coords(rows, cols, H):
    """The source coordinate of every destination pixel as np_easu.remap_homography forms it (FSR.cl:423-430)."""
    H = np.asarray(H, f32).reshape(9)
    yy, xx = np.mgrid[0:rows, 0:cols]
    fx = xx.astype(f32); fy = yy.astype(f32)
    dz = f32(1) / (_fma(H[6], fx, H[7] * fy) + H[8])
    ox = (_fma(H[0], fx, H[1] * fy) + H[2]) * dz - fx
    oy = (_fma(H[3], fx, H[4] * fy) + H[5]) * dz - fy
    return fx + ox, fy + oy


def remap_homography(src, H, bg, yuv):
    subx, suby = homography_coords(src.shape[0], src.shape[1], H)
    return remap_tail(src, subx, suby, bg, yuv)[0]


def interior_mask(rows, cols, H):
    """Which destination pixels of a homography remap reach the EASU weights (True) -- the rest are border-band copies or background."""
    subx, suby = homography_coords(rows, cols, H)
    sx = np.trunc(np.clip(subx, -2e9, 2e9)).astype(np.int64)
    sy = np.trunc(np.clip(suby, -2e9, 2e9)).astype(np.int64)
    return ~((sx < 1) | (sy < 1) | (sx >= cols - 4) | (sy >= rows - 4))
