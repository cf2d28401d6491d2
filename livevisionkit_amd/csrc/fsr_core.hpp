// The FSR 1 EASU pass (FidelityFX FsrEasuF; specification: tests/np_fsr.py) as far as it does not depend on what a texel is or
// where a pixel goes, written once for the kernels of fsr.hip (packed 3- and 4-channel frames), fsr_gray.hip (one channel) and fsr_planes.hpp (the
// planes of an OBS video format): the direction / length analysis, which sees only the lumas of the 12 taps, the weight of a tap from its offset, the
// tap order, the tile walk (a tile's column side, the fill of its LDS stage, the 12-tap gather of a row), and the host's side of a launch: the
// geometry, the region check, the grid and the measure of a tile's source footprint against the stage.  Every operation is rounded on its own
// (-ffp-contract=off).
#pragma once

#include "cas_core.hpp"
#include "lvk_hip.h"

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

// FsrEasuF's accumulation order of the 12 taps t[dy + 1][dx + 1] (dx, dy in -1 .. 2; the four corners are not used): b c i j f e k l h g o n, each
// handed to tap(dx, dy, texel)
template <class T, class Tap>
__device__ __forceinline__ void easu_taps(const T (&t)[4][4], Tap tap)
{
    tap(0.0f, -1.0f, t[0][1]);
    tap(1.0f, -1.0f, t[0][2]);
    tap(-1.0f, 1.0f, t[2][0]);
    tap(0.0f, 1.0f, t[2][1]);
    tap(0.0f, 0.0f, t[1][1]);
    tap(-1.0f, 0.0f, t[1][0]);
    tap(1.0f, 1.0f, t[2][2]);
    tap(2.0f, 1.0f, t[2][3]);
    tap(2.0f, 0.0f, t[1][3]);
    tap(1.0f, 0.0f, t[1][2]);
    tap(1.0f, 2.0f, t[3][2]);
    tap(0.0f, 2.0f, t[3][1]);
}

// The three-channel pixel function, on texels (r, g, b, luma): shared by fsr.hip and the plane kernels of fsr_planes.hpp.
// FsrEasuF from the 12 taps t and the fraction (ppx, ppy) of pp
__device__ __forceinline__ float3 easu(const float4 (&t)[4][4], float ppx, float ppy)
{
    const float4 f = t[1][1], g = t[1][2], j = t[2][1], k = t[2][2];
    const EasuLobe lobe = easu_analyse(t[0][1].w, t[0][2].w, t[1][0].w, f.w, g.w, t[1][3].w, t[2][0].w, j.w, k.w, t[2][3].w, t[3][1].w, t[3][2].w, ppx, ppy);
    float3 ac = make_float3(0.0f, 0.0f, 0.0f);
    float aw = 0.0f;
    easu_taps(t, [&](float ox, float oy, float4 c) {   // FsrEasuTapF
        const float w = easu_weight(ox, oy, ppx, ppy, lobe);
        ac.x = ac.x + c.x * w;
        ac.y = ac.y + c.y * w;
        ac.z = ac.z + c.z * w;
        aw = aw + w;
    });
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

// what every EASU kernel is told of a launch
struct FsrGeo
{
    int rows, cols;                        // the frame
    int rx, ry;                            // the region's origin
    int out_rows, out_cols;
    float c0x, c0y, c0z, c0w;              // FsrEasuCon's con0 (con1 .. con3 only place the texels, which are integers here)
};

// the position of output pixel ip in the region (FsrEasuCon's con0: scale and bias), as every kernel and the host compute it
__host__ __device__ __forceinline__ float pp_of(int ip, float scale, float bias) { return (float)ip * scale + bias; }

// ---- The tile walk.  The texel of a tap is (fp.x + rx + dx, fp.y + ry + dy), dx, dy in -1 .. 2, clamped to the frame: the shader's point sampler picks
// exactly that texel (declared choice 6, pinned by tests/test_fsr_spec.py), so no texture coordinate is formed.  T is a kernel's texel (float4 or float)
// and fetch(sx, sy) gives the texel at the clamped frame coordinates (sx, sy).  A staged kernel reads the tile's source footprint (its fp range plus the
// -1 .. 2 taps) through fetch once into LDS; a direct kernel calls fetch per tap.

// the column side of a tile that starts at output column x0, for the lane that computes column x
struct EasuCol
{
    float ppx; int fx;                     // the fraction and the floor of pp.x at x
    int fx0, sw;                           // the tile's first fp.x and its staged columns: fx0 - 1 .. fx1 + 2
};

__device__ __forceinline__ EasuCol easu_col(const FsrGeo& a, int x0, int x)
{
    const float ppx_full = pp_of(x, a.c0x, a.c0z), fpx = floorf(ppx_full);
    // the tile's first and last fp.x: pp grows with x, and rounding keeps that order
    const int fx0 = (int)floorf(pp_of(x0, a.c0x, a.c0z));
    const int fx1 = (int)floorf(pp_of(min(x0 + kTileW, a.out_cols) - 1, a.c0x, a.c0z));
    return EasuCol{ppx_full - fpx, (int)fpx, fx0, fx1 - fx0 + 4};
}

// fills the stage of the tile row that starts at output row y0 (all 256 threads, ends in the barrier); returns the tile row's first fp.y
template <class T, class Fetch>
__device__ __forceinline__ int easu_stage_fill(T* stage, const FsrGeo& a, const EasuCol& c, int y0, int tid, Fetch fetch)
{
    const int fy0 = (int)floorf(pp_of(y0, a.c0y, a.c0w));
    const int fy1 = (int)floorf(pp_of(min(y0 + kTileH, a.out_rows) - 1, a.c0y, a.c0w));
    const int sw = c.sw, sh = fy1 - fy0 + 4;
    for (int k = tid; k < sw * sh; k += 256)
    {
        const int ty = k / sw, tx = k - ty * sw;
        stage[k] = fetch(min(max(c.fx0 - 1 + a.rx + tx, 0), a.cols - 1), min(max(fy0 - 1 + a.ry + ty, 0), a.rows - 1));
    }
    __syncthreads();
    return fy0;
}

// the 12 taps of output row y into t[dy + 1][dx + 1], the four unused corners zero; returns the fraction of pp.y
template <bool kStaged, class T, class Fetch>
__device__ __forceinline__ float easu_gather(T (&t)[4][4], const T* stage, const FsrGeo& a, const EasuCol& c, int fy0, int y, Fetch fetch)
{
    const float ppy_full = pp_of(y, a.c0y, a.c0w), fpy = floorf(ppy_full);
    const int fy = (int)fpy;
    const T* s = stage + (fy - fy0) * c.sw + (c.fx - c.fx0);
    int cx[4];
#pragma unroll
    for (int dx = 0; dx < 4; dx++) cx[dx] = min(max(c.fx + a.rx + dx - 1, 0), a.cols - 1);
#pragma unroll
    for (int dy = 0; dy < 4; dy++)
    {
        const int sy = min(max(fy + a.ry + dy - 1, 0), a.rows - 1);
#pragma unroll
        for (int dx = 0; dx < 4; dx++)
            if ((dy == 0 || dy == 3) && (dx == 0 || dx == 3)) t[dy][dx] = T{};
            else if (kStaged) t[dy][dx] = s[dy * c.sw + dx];
            else t[dy][dx] = fetch(cx[dx], sy);
    }
    return ppy_full - fpy;
}

// ---- The host's side of a launch

constexpr int kStageBytes = 40 * 1024;     // LDS budget of the staged path: four blocks per CU
template <class T> constexpr int kStageTexels = kStageBytes / (int)sizeof(T);

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

// 0 when the largest tile footprint of scaling a rw x rh region to out_cols x out_rows fits a stage of `texels` (staged), 1 when not (direct)
inline int fsr_stage_fits(int rw, int rh, int out_rows, int out_cols, int texels)
{
    float con[16];
    if (lvk_hip_fsr_easu_const(rw, rh, 1, 1, out_cols, out_rows, con) != LVK_HIP_OK) return LVK_HIP_ERR_ARG;
    const long long sw = max_fp_span(out_cols, kTileW, con[0], con[2]) + 3LL, sh = max_fp_span(out_rows, kTileH, con[1], con[3]) + 3LL;
    return sw * sh <= texels ? 0 : 1;
}

// what every entry asks of its region: a non-empty rectangle inside the frame
inline bool fsr_region_ok(const int region_xywh[4], int rows, int cols)
{
    const int rx = region_xywh[0], ry = region_xywh[1], rw = region_xywh[2], rh = region_xywh[3];
    return rx >= 0 && ry >= 0 && rw > 0 && rh > 0 && (long long)rx + rw <= cols && (long long)ry + rh <= rows;
}

inline FsrGeo fsr_geo(int rows, int cols, const int region_xywh[4], int out_rows, int out_cols)
{
    float con[16];
    lvk_hip_fsr_easu_const(region_xywh[2], region_xywh[3], cols, rows, out_cols, out_rows, con);
    return FsrGeo{rows, cols, region_xywh[0], region_xywh[1], out_rows, out_cols, con[0], con[1], con[2], con[3]};
}

// one block per tile across, a grid-stride loop over the rows of tiles
inline dim3 fsr_grid(const FsrGeo& a)
{
    return dim3((unsigned)((a.out_cols + kTileW - 1) / kTileW), (unsigned)std::min((a.out_rows + kTileH - 1) / kTileH, 65535));
}

} // namespace ffx
