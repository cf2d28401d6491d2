// The FSR filter's EASU pass (fsr.hip) on ONE-channel frames (8UC1, VideoFrame::GRAY) for gfx950: the kernels behind lvk_hip_fsr_easu_gray.
//
// The plugin runs FSR as an RGBA effect, so there is no one-channel program to copy.  DEFINITION: channel 0 of the
// three-channel specification (tests/np_fsr.py) on (g, g, g), which is the same for BGR, RGB and YUV.  The geometry is that of
// lvk_hip_fsr_geometry: a crop region, taps clamped to the frame, any output size.  The direction / length analysis and the tap weights are the
// functions of fsr_core.hpp that k_fsr_easu<C, kStaged> calls; here they feed one accumulator and one de-ringing clamp instead of three.  The luma
// of a grey texel, 0.5 v + (0.5 v + v) in binary32, is 2 v exactly for all 256 bytes (tests/test_ffx_gray_spec.py pins it) and is formed as v + v.
//
// One kernel, k_fsr_easu_gray<kStaged>, with the tile and the two tap paths of k_fsr_easu:
//   staged   the tile's source footprint is read once into LDS as one float per texel (the luma is one addition per tap: staging it too would
//            double the LDS reads and halve the footprints that fit).  A texel is 4 bytes, not 16, so four times the footprint fits the same
//            40 KiB and most downscales stay staged.
//   direct   each tap reads its byte from the frame (footprints beyond kStageTexels).
// Output: the four lanes whose bytes share an aligned dword of the destination row hand them to the first of the four (wave shuffles), which
// stores the dword; lanes whose dword is cut by the tile's or the row's end store their byte.  No byte outside out_cols of a row is written.
#include "lvk_hip_internal.hpp"
#include "fsr_core.hpp"

#include <algorithm>
#include <cstdint>

namespace {

using namespace ffx;

constexpr int kStageTexels = 10240;        // LDS budget of the staged path: 40 KiB of float, four blocks per CU

struct EasuGrayArgs
{
    const uint8_t* src;
    long long src_step;
    int rows, cols;                        // the frame
    int rx, ry;                            // the region's origin
    uint8_t* dst;
    long long dst_step;
    int out_rows, out_cols;
    float c0x, c0y, c0z, c0w;              // FsrEasuCon's con0
};

// FsrEasuF with one channel, from the 12 taps t[dy + 1][dx + 1] (dx, dy in -1 .. 2; the four corners are not used) and the fraction of pp
__device__ __forceinline__ float easu_gray(const float (&t)[4][4], float ppx, float ppy)
{
    const float b = t[0][1], c = t[0][2], e = t[1][0], f = t[1][1], g = t[1][2], h = t[1][3];
    const float i = t[2][0], j = t[2][1], k = t[2][2], l = t[2][3], n = t[3][1], o = t[3][2];
    const EasuLobe lobe = easu_analyse(b + b, c + c, e + e, f + f, g + g, h + h, i + i, j + j, k + k, l + l, n + n, o + o, ppx, ppy);
    float ac = 0.0f, aw = 0.0f;
    auto tap = [&](float ox, float oy, float v) {
        const float w = easu_weight(ox, oy, ppx, ppy, lobe);
        ac = ac + v * w;
        aw = aw + w;
    };
    tap(0.0f, -1.0f, b);                               // FsrEasuF's order
    tap(1.0f, -1.0f, c);
    tap(-1.0f, 1.0f, i);
    tap(0.0f, 1.0f, j);
    tap(0.0f, 0.0f, f);
    tap(-1.0f, 0.0f, e);
    tap(1.0f, 1.0f, k);
    tap(2.0f, 1.0f, l);
    tap(2.0f, 0.0f, h);
    tap(1.0f, 0.0f, g);
    tap(1.0f, 2.0f, o);
    tap(0.0f, 2.0f, n);
    const float inv = 1.0f / aw;                       // correctly rounded (ARcpF1 on OpenGL)
    const float mn = __builtin_fminf(__builtin_fminf(__builtin_fminf(f, g), j), k);
    const float mx = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(f, g), j), k);
    return __builtin_fminf(mx, __builtin_fmaxf(mn, ac * inv));
}

// One output row of a wave: lane `lane` holds the byte of column x (live: x < out_cols).  Called by all 64 lanes.
__device__ __forceinline__ void store_row(const EasuGrayArgs& a, int x, int y, int lane, bool live, uint32_t byte)
{
    uint8_t* p = a.dst + (long long)y * a.dst_step + x;
    const int al = (int)(reinterpret_cast<uintptr_t>(p) & 3u);
    const uint32_t b1 = __shfl_down(byte, 1), b2 = __shfl_down(byte, 2), b3 = __shfl_down(byte, 3);
    // the dword that holds this lane's byte starts at lane - al, column x - al: whole when its four bytes are live lanes of this wave
    const bool whole = lane - al >= 0 && lane - al + 3 < 64 && x - al + 3 < a.out_cols;
    if (!live) return;
    if (!whole) *p = (uint8_t)byte;
    else if (al == 0) *reinterpret_cast<uint32_t*>(p) = byte | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

template <bool kStaged>
__global__ __launch_bounds__(256)
void k_fsr_easu_gray(EasuGrayArgs a)
{
    __shared__ float stage[kStaged ? kStageTexels : 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kTileW;
    const int x = x0 + lane;
    const bool live = x < a.out_cols;
    // (a lane beyond the row's end computes the row's last column, so that it stays inside the footprint and takes part in the shuffles)
    const float ppx_full = pp_of(min(x, a.out_cols - 1), a.c0x, a.c0z);
    const float fpx = floorf(ppx_full), ppx = ppx_full - fpx;
    const int fx = (int)fpx;
    // the tile's first and last fp.x: pp grows with x, and rounding keeps that order
    const int fx0 = (int)floorf(pp_of(x0, a.c0x, a.c0z));
    const int fx1 = (int)floorf(pp_of(min(x0 + kTileW, a.out_cols) - 1, a.c0x, a.c0z));
    const int sw = fx1 - fx0 + 4;                                  // staged columns: fp.x - 1 .. fp.x + 2

    for (int y0 = blockIdx.y * kTileH; y0 < a.out_rows; y0 += gridDim.y * kTileH)
    {
        int fy0 = 0;
        if (kStaged)
        {
            fy0 = (int)floorf(pp_of(y0, a.c0y, a.c0w));
            const int fy1 = (int)floorf(pp_of(min(y0 + kTileH, a.out_rows) - 1, a.c0y, a.c0w));
            const int sh = fy1 - fy0 + 4;
            for (int k = tid; k < sw * sh; k += 256)
            {
                const int ty = k / sw, tx = k - ty * sw;
                const int sx = min(max(fx0 - 1 + a.rx + tx, 0), a.cols - 1);
                const int sy = min(max(fy0 - 1 + a.ry + ty, 0), a.rows - 1);
                stage[k] = unit_of((float)a.src[(long long)sy * a.src_step + sx]);
            }
            __syncthreads();
        }
#pragma unroll 1
        for (int j = 0; j < kRowsPerWave; j++)
        {
            const int y = y0 + wave * kRowsPerWave + j;
            if (y >= a.out_rows) break;                             // (wave-uniform)
            const float ppy_full = pp_of(y, a.c0y, a.c0w);
            const float fpy = floorf(ppy_full), ppy = ppy_full - fpy;
            const int fy = (int)fpy;
            float t[4][4];
            if (kStaged)
            {
                const float* s = stage + (fy - fy0) * sw + (fx - fx0);
#pragma unroll
                for (int dy = 0; dy < 4; dy++)
#pragma unroll
                    for (int dx = 0; dx < 4; dx++)
                        if ((dy == 0 || dy == 3) && (dx == 0 || dx == 3)) t[dy][dx] = 0.0f;
                        else t[dy][dx] = s[dy * sw + dx];
            }
            else
            {
                int cx[4];
#pragma unroll
                for (int dx = 0; dx < 4; dx++) cx[dx] = min(max(fx + a.rx + dx - 1, 0), a.cols - 1);
#pragma unroll
                for (int dy = 0; dy < 4; dy++)
                {
                    const int sy = min(max(fy + a.ry + dy - 1, 0), a.rows - 1);
                    const uint8_t* row = a.src + (long long)sy * a.src_step;
#pragma unroll
                    for (int dx = 0; dx < 4; dx++)
                        if ((dy == 0 || dy == 3) && (dx == 0 || dx == 3)) t[dy][dx] = 0.0f;
                        else t[dy][dx] = unit_of((float)row[cx[dx]]);
                }
            }
            store_row(a, x, y, lane, live, to_byte(easu_gray(t, ppx, ppy)));
        }
        if (kStaged) __syncthreads();                               // the stage is reused by the next row of tiles
    }
}

} // namespace

extern "C" {

int lvk_hip_fsr_easu_gray_path(int rw, int rh, int out_rows, int out_cols)
{
    float con[16];
    if (lvk_hip_fsr_easu_const(rw, rh, 1, 1, out_cols, out_rows, con) != LVK_HIP_OK) return LVK_HIP_ERR_ARG;
    const long long sw = max_fp_span(out_cols, kTileW, con[0], con[2]) + 3LL, sh = max_fp_span(out_rows, kTileH, con[1], con[3]) + 3LL;
    return sw * sh <= kStageTexels ? 0 : 1;
}

int lvk_hip_fsr_easu_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, const int region_xywh[4], void* d_dst,
                          int dst_step, int out_rows, int out_cols)
{
    LVK_HIP_ENTRY(ctx);
    LVK_HIP_REQUIRE(ctx, d_src && d_dst && region_xywh && rows > 0 && cols > 0 && out_rows > 0 && out_cols > 0);
    const int rx = region_xywh[0], ry = region_xywh[1], rw = region_xywh[2], rh = region_xywh[3];
    if (!(rx >= 0 && ry >= 0 && rw > 0 && rh > 0 && (long long)rx + rw <= cols && (long long)ry + rh <= rows))
        return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_fsr_easu_gray: the region must be a non-empty rectangle inside the frame");
    LVK_HIP_REQUIRE(ctx, src_step >= cols && dst_step >= out_cols);
    if (lvk_pitched_overlap(d_src, src_step, rows, cols, d_dst, dst_step, out_rows, out_cols)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_fsr_easu_gray: the source and destination overlap");

    float con[16];
    lvk_hip_fsr_easu_const(rw, rh, cols, rows, out_cols, out_rows, con);
    const EasuGrayArgs a{(const uint8_t*)d_src, (long long)src_step, rows, cols, rx, ry, (uint8_t*)d_dst, (long long)dst_step, out_rows, out_cols,
                         con[0], con[1], con[2], con[3]};
    const bool staged = lvk_hip_fsr_easu_gray_path(rw, rh, out_rows, out_cols) == 0;
    const dim3 grid((unsigned)((out_cols + kTileW - 1) / kTileW), (unsigned)std::min((out_rows + kTileH - 1) / kTileH, 65535));
    if (staged) hipLaunchKernelGGL((k_fsr_easu_gray<true>), grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_fsr_easu_gray<false>), grid, dim3(256), 0, ctx->stream, a);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

} // extern "C"
