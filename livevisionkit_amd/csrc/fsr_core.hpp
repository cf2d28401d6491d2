// The channel-agnostic part of the FSR 1 EASU pass (FidelityFX FsrEasuF; specification: tests/np_fsr.py), written once for
// the kernels of fsr.hip (packed 3- and 4-channel frames) and fsr_gray.hip (one channel): the direction / length analysis, which sees only the
// lumas of the 12 taps, the weight of a tap from its offset, and the host's measure of a tile's source footprint.  Every operation is rounded on
// its own (-ffp-contract=off).
#pragma once

#include "cas_core.hpp"

#include <algorithm>
#include <cmath>

namespace ffx {

// every EASU kernel: a block of 256 threads owns one output tile, lane l of wave w computes column l of rows 4w .. 4w + 3
constexpr int kTileW = 64;                 // output columns per tile (one per lane)
constexpr int kTileH = 16;                 // output rows per tile (4 per wave)
constexpr int kRowsPerWave = kTileH / 4;

__device__ __forceinline__ float lo_rcp(float v) { return as_f(0x7ef07ebbu - as_u(v)); }
__device__ __forceinline__ float lo_rsq(float v) { return as_f(0x5f347d74u - (as_u(v) >> 1)); }

// FsrEasuSetF: one bilinear corner's contribution to the direction and the length
__device__ __forceinline__ void easu_set(float& dirx, float& diry, float& len, float w, float lA, float lB, float lC, float lD, float lE)
{
    const float dc = lD - lC, cb = lC - lB;
    float lenx = lo_rcp(__builtin_fmaxf(__builtin_fabsf(dc), __builtin_fabsf(cb)));
    const float dx = lD - lB;
    dirx = dirx + dx * w;
    lenx = sat(__builtin_fabsf(dx) * lenx);
    lenx = lenx * lenx;
    len = len + lenx * w;
    const float ec = lE - lC, ca = lC - lA;
    float leny = lo_rcp(__builtin_fmaxf(__builtin_fabsf(ec), __builtin_fabsf(ca)));
    const float dy = lE - lA;
    diry = diry + dy * w;
    leny = sat(__builtin_fabsf(dy) * leny);
    leny = leny * leny;
    len = len + leny * w;
}

// what the analysis hands to the taps: the unit direction, the anisotropic stretch, the negative lobe and the clipping point of the window
struct EasuLobe { float dirx, diry, len2x, len2y, lob, clp; };

// The first half of FsrEasuF: from the lumas of the 12 taps (b c / e f g h / i j k l / n o) and the fraction (ppx, ppy) of pp
__device__ __forceinline__ EasuLobe easu_analyse(float bL, float cL, float eL, float fL, float gL, float hL, float iL, float jL, float kL, float lL,
                                                 float nL, float oL, float ppx, float ppy)
{
    float dirx = 0.0f, diry = 0.0f, len = 0.0f;
    easu_set(dirx, diry, len, (1.0f - ppx) * (1.0f - ppy), bL, eL, fL, gL, jL);
    easu_set(dirx, diry, len, ppx * (1.0f - ppy), cL, fL, gL, hL, kL);
    easu_set(dirx, diry, len, (1.0f - ppx) * ppy, fL, iL, jL, kL, nL);
    easu_set(dirx, diry, len, ppx * ppy, gL, jL, kL, lL, oL);
    const float dir2x = dirx * dirx, dir2y = diry * diry;
    float dirr = dir2x + dir2y;
    const bool zro = dirr < (1.0f / 32768.0f);
    dirr = zro ? 1.0f : lo_rsq(dirr);
    dirx = zro ? 1.0f : dirx;
    dirx = dirx * dirr;
    diry = diry * dirr;
    len = len * 0.5f;
    len = len * len;
    const float stretch = (dirx * dirx + diry * diry) * lo_rcp(__builtin_fmaxf(__builtin_fabsf(dirx), __builtin_fabsf(diry)));
    const float len2x = 1.0f + (stretch - 1.0f) * len;
    const float len2y = 1.0f + -0.5f * len;
    const float lob = 0.5f + -0.29f * len;             // (float)((1/4 - 0.04) - 0.5)
    return EasuLobe{dirx, diry, len2x, len2y, lob, lo_rcp(lob)};
}

// The weight half of FsrEasuTapF for the tap at (ox, oy) from 'f'
__device__ __forceinline__ float easu_weight(float ox, float oy, float ppx, float ppy, const EasuLobe& e)
{
    const float offx = ox - ppx, offy = oy - ppy;
    float vx = (offx * e.dirx) + (offy * e.diry);
    float vy = (offx * (-e.diry)) + (offy * e.dirx);
    vx = vx * e.len2x;
    vy = vy * e.len2y;
    const float d2 = __builtin_fminf(vx * vx + vy * vy, e.clp);
    float wb = 0.4f * d2 + -1.0f;
    float wa = e.lob * d2 + -1.0f;
    wb = wb * wb;
    wa = wa * wa;
    wb = 1.5625f * wb + -0.5625f;
    return wb * wa;
}

// The three-channel pixel function, on texels (r, g, b, luma): shared by fsr.hip and the plane kernels of fsr_planes.hpp.
// FsrEasuTapF for the tap at (ox, oy) from 'f'
__device__ __forceinline__ void easu_tap(float3& ac, float& aw, float ox, float oy, float ppx, float ppy, const EasuLobe& lobe, float4 c)
{
    const float w = easu_weight(ox, oy, ppx, ppy, lobe);
    ac.x = ac.x + c.x * w;
    ac.y = ac.y + c.y * w;
    ac.z = ac.z + c.z * w;
    aw = aw + w;
}

// FsrEasuF from the 12 taps t[dy + 1][dx + 1] (dx, dy in -1 .. 2; the four corners are not used) and the fraction (ppx, ppy) of pp
__device__ __forceinline__ float3 easu(const float4 (&t)[4][4], float ppx, float ppy)
{
    const float4 b = t[0][1], c = t[0][2], e = t[1][0], f = t[1][1], g = t[1][2], h = t[1][3];
    const float4 i = t[2][0], j = t[2][1], k = t[2][2], l = t[2][3], n = t[3][1], o = t[3][2];
    const EasuLobe lobe = easu_analyse(b.w, c.w, e.w, f.w, g.w, h.w, i.w, j.w, k.w, l.w, n.w, o.w, ppx, ppy);
    float3 ac = make_float3(0.0f, 0.0f, 0.0f);
    float aw = 0.0f;
    easu_tap(ac, aw, 0.0f, -1.0f, ppx, ppy, lobe, b);
    easu_tap(ac, aw, 1.0f, -1.0f, ppx, ppy, lobe, c);
    easu_tap(ac, aw, -1.0f, 1.0f, ppx, ppy, lobe, i);
    easu_tap(ac, aw, 0.0f, 1.0f, ppx, ppy, lobe, j);
    easu_tap(ac, aw, 0.0f, 0.0f, ppx, ppy, lobe, f);
    easu_tap(ac, aw, -1.0f, 0.0f, ppx, ppy, lobe, e);
    easu_tap(ac, aw, 1.0f, 1.0f, ppx, ppy, lobe, k);
    easu_tap(ac, aw, 2.0f, 1.0f, ppx, ppy, lobe, l);
    easu_tap(ac, aw, 2.0f, 0.0f, ppx, ppy, lobe, h);
    easu_tap(ac, aw, 1.0f, 0.0f, ppx, ppy, lobe, g);
    easu_tap(ac, aw, 1.0f, 2.0f, ppx, ppy, lobe, o);
    easu_tap(ac, aw, 0.0f, 2.0f, ppx, ppy, lobe, n);
    const float inv = 1.0f / aw;                       // correctly rounded (ARcpF1 on OpenGL)
    const float mnr = __builtin_fminf(__builtin_fminf(__builtin_fminf(f.x, g.x), j.x), k.x);
    const float mng = __builtin_fminf(__builtin_fminf(__builtin_fminf(f.y, g.y), j.y), k.y);
    const float mnb = __builtin_fminf(__builtin_fminf(__builtin_fminf(f.z, g.z), j.z), k.z);
    const float mxr = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(f.x, g.x), j.x), k.x);
    const float mxg = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(f.y, g.y), j.y), k.y);
    const float mxb = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(f.z, g.z), j.z), k.z);
    return make_float3(__builtin_fminf(mxr, __builtin_fmaxf(mnr, ac.x * inv)), __builtin_fminf(mxg, __builtin_fmaxf(mng, ac.y * inv)),
                       __builtin_fminf(mxb, __builtin_fmaxf(mnb, ac.z * inv)));
}

// the position of output pixel ip in the region (FsrEasuCon's con0: scale and bias), as every kernel and the host compute it
__host__ __device__ __forceinline__ float pp_of(int ip, float scale, float bias) { return (float)ip * scale + bias; }

// The largest fp span (last - first + 1) of any tile-sized run of outputs 0 .. n - 1, with the kernels' float32 arithmetic (host only).
inline int max_fp_span(int n, int tile, float scale, float bias)
{
    int worst = 0;
    for (int i0 = 0; i0 < n; i0 += tile)
    {
        const int i1 = std::min(i0 + tile, n) - 1;
        const int f0 = (int)std::floor(pp_of(i0, scale, bias)), f1 = (int)std::floor(pp_of(i1, scale, bias));
        worst = std::max(worst, f1 - f0 + 1);
    }
    return worst;
}

} // namespace ffx
