"""Independent numpy restatement of the OBS plugin's CAS filter (contrast adaptive sharpening): CASFilter / CASEffect on the host, the
FidelityFX CasFilter of cas.effect (CAS_SLOW and CAS_BETTER_DIAGONALS defined, CAS_GO_SLOWER not, no scaling) on the pixels.

Every operation is float32 and rounded on its own (no fused multiply-adds); the approximate reciprocals and square root are the FidelityFX
bit tricks on the float's uint32 pattern, not the hardware's.  Per pixel and per channel c (CAS_SLOW: one weight per channel):

  load       x = u8 / 255, correctly rounded; neighbours outside the frame read as 0 (D3D11's out-of-bounds Load)
  window     a b c / d e f / g h i around e
  min / max  mn = min(d, e, f, b, h) + min(that, a, c, g, i);  mx likewise with max (CAS_BETTER_DIAGONALS)
  amp        lo_sqrt(sat(min(mn, 2 - mx) * lo_rcp(mx)))
  weight     w = amp * peak,  peak = -(1 / (5 s + ((-8) s + 8)))  (CasSetup on the host, s = clamp(sharpness, 0, 1))
  out        sat(((((b w + d w) + f w) + h w) + e) * med_rcp(1 + 4 w))
  store      rint(out * 255), round half to even; a 4th channel is written as 255 (the shader returns float4(col, 1.0))

The float64 `textbook_cas` (exact reciprocal and square root, no float32 rounding) is a bound for the restatement, not a specification.
"""
from fractions import Fraction

import numpy as np

f32 = np.float32
u32 = np.uint32
FMT_BGR, FMT_BGRA, FMT_RGB, FMT_RGBA, FMT_YUV, FMT_GRAY = 0, 1, 2, 3, 4, 5
CHANNELS = {FMT_BGR: 3, FMT_RGB: 3, FMT_YUV: 3, FMT_BGRA: 4, FMT_RGBA: 4}


def _as_f32(bits):
    return np.asarray(bits, dtype=u32).view(f32)


def _as_u32(v):
    return np.asarray(v, dtype=f32).view(u32)


LO_RCP_BITS = 0x7ef07ebb
MED_RCP_BITS = 0x7ef19fff


def lo_rcp(v):
    """APrxLoRcpF1: as_float(0x7ef07ebb - as_uint(v))."""
    return _as_f32(u32(LO_RCP_BITS) - _as_u32(v))


def lo_sqrt(v):
    """APrxLoSqrtF1: as_float((as_uint(v) >> 1) + 0x1fbc4639)."""
    return _as_f32((_as_u32(v) >> u32(1)) + u32(0x1fbc4639))


def med_rcp(v):
    """APrxMedRcpF1: r = as_float(0x7ef19fff - as_uint(v)); r * ((-r) * v + 2), each operation rounded on its own."""
    v = np.asarray(v, dtype=f32)
    r = _as_f32(u32(MED_RCP_BITS) - _as_u32(v))
    return r * ((-r) * v + f32(2))


def sat(v):
    return np.minimum(np.maximum(v, f32(0)), f32(1))


def peak_of(sharpness):
    """CasSetup's const1.x: ALerpF1(8, 5, s) = 5 s + ((-8) s + 8) on the CPU, then -ARcpF1, all float32."""
    s = f32(min(max(f32(sharpness), f32(0)), f32(1)))
    lerp = f32(f32(5) * s) + f32(f32(f32(-8) * s) + f32(8))
    return f32(-(f32(1) / lerp))


def _u8_to_unit():
    """The 256 correctly rounded float32 values of u / 255 (exact rational comparison of the two float32 neighbours)."""
    out = np.empty(256, f32)
    for u in range(256):
        q = Fraction(u, 255)
        lo = f32(u / 255.0)
        cands = [lo, np.nextafter(lo, f32(-1)), np.nextafter(lo, f32(2))]
        out[u] = min(cands, key=lambda c: (abs(Fraction(float(c)) - q), int(_as_u32(c)) & 1))
    return out


UNIT = _u8_to_unit()


def _window(x):
    """The nine neighbours of every pixel of x [rows, cols, ch] with zero outside the frame: (a, b, c, d, e, f, g, h, i)."""
    rows, cols = x.shape[:2]
    p = np.zeros((rows + 2, cols + 2) + x.shape[2:], f32)
    p[1:-1, 1:-1] = x
    return [p[dy:dy + rows, dx:dx + cols] for dy in range(3) for dx in range(3)]


def soft_min(a, b, c, d, e, f, g, h, i):
    """The plus-shaped minimum added to the minimum over the whole window (CAS_BETTER_DIAGONALS): twice the soft minimum."""
    mn = np.minimum(np.minimum(np.minimum(d, e), f), np.minimum(b, h))
    return mn + np.minimum(np.minimum(mn, a), np.minimum(np.minimum(c, g), i))


def soft_max(a, b, c, d, e, f, g, h, i):
    mx = np.maximum(np.maximum(np.maximum(d, e), f), np.maximum(b, h))
    return mx + np.maximum(np.maximum(mx, a), np.maximum(np.maximum(c, g), i))


def weighted_sum(b, d, f, h, e, w):
    """b w + d w + f w + h w + e, summed left to right."""
    return (((b * w + d * w) + f * w) + h * w) + e


def cas_unit(x, peak):
    """CasFilter on a float32 [rows, cols, ch] frame of values in [0, 1]; returns the saturated float32 result."""
    a, b, c, d, e, f, g, h, i = _window(np.asarray(x, f32))
    mn = soft_min(a, b, c, d, e, f, g, h, i)
    mx = soft_max(a, b, c, d, e, f, g, h, i)
    amp = lo_sqrt(sat(np.minimum(mn, f32(2) - mx) * lo_rcp(mx)))
    w = amp * f32(peak)
    return sat(weighted_sum(b, d, f, h, e, w) * med_rcp(f32(1) + f32(4) * w))


def cas(img, sharpness=0.8):
    """The CAS filter on a uint8 [rows, cols, 3 | 4] frame: channels 0-2 sharpened, a 4th channel written as 255."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (3, 4)
    out = np.empty_like(img)
    y = cas_unit(UNIT[img[..., :3]], peak_of(sharpness))
    out[..., :3] = np.rint(y * f32(255)).astype(np.uint8)
    if img.shape[2] == 4:
        out[..., 3] = 255
    return out


def textbook_cas(img, sharpness=0.8):
    """A float64 CAS with exact division and square root (same window, zero border, CAS_BETTER_DIAGONALS): the bound of the tests."""
    x = np.asarray(img, np.float64)[..., :3] / 255.0
    rows, cols = x.shape[:2]
    p = np.zeros((rows + 2, cols + 2, 3))
    p[1:-1, 1:-1] = x
    a, b, c, d, e, f, g, h, i = [p[dy:dy + rows, dx:dx + cols] for dy in range(3) for dx in range(3)]
    mn = np.minimum.reduce([d, e, f, b, h])
    mx = np.maximum.reduce([d, e, f, b, h])
    mn = mn + np.minimum.reduce([mn, a, c, g, i])
    mx = mx + np.maximum.reduce([mx, a, c, g, i])
    with np.errstate(divide="ignore", invalid="ignore"):
        amp = np.sqrt(np.clip(np.where(mx > 0, np.minimum(mn, 2 - mx) / mx, 0.0), 0, 1))
    s = min(max(float(sharpness), 0.0), 1.0)
    w = amp * (-1.0 / (8.0 - 3.0 * s))
    y = np.clip((b * w + d * w + f * w + h * w + e) / (1 + 4 * w), 0, 1)
    out = np.array(img, np.uint8, copy=True)
    out[..., :3] = np.rint(y * 255).astype(np.uint8)
    if out.shape[2] == 4:
        out[..., 3] = 255
    return out
