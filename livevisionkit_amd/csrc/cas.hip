// The OBS plugin's CAS filter (contrast adaptive sharpening: CASFilter / CASEffect, the FidelityFX CasFilter of cas.effect with CAS_SLOW
// and CAS_BETTER_DIAGONALS) on the MI355X, out of place on a packed 3- or 4-channel frame.  Specification: tests/np_cas.py and DESIGN.md
// section 14.
//
// One kernel, k_cas<C>, on the context's stream.  A block of 256 threads owns a 64 x 16 pixel tile:
//   load     the tile plus a one-pixel halo is read row by row as aligned dwords (only dwords that hold a byte of the frame), each byte is
//            converted once to u / 255 (correctly rounded) and staged as float32 in LDS; outside the frame the tile holds 0.  A 4-channel
//            frame's 4th byte is not staged.
//   compute  wave w walks rows 4w .. 4w + 3 of the tile, one pixel column per lane, with a 3 x 3 x 3 register window that takes one new
//            tile row (3 pixels) per output row.  The arithmetic is the specification's, unfused, with the FidelityFX bit tricks
//            (cas_core.hpp).
//   store    the output bytes go to a second LDS tile laid out at the destination's byte alignment, then out as aligned dwords; only the
//            partial dwords at the two ends of a row segment are written byte by byte.  No byte outside cols * C of a row is written.
#include "lvk_hip_internal.hpp"
#include "cas_core.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

constexpr int kTileW = 64;                 // pixels per tile row (one per lane)
constexpr int kTileH = 16;                 // rows per tile (4 per wave)
constexpr int kRowsPerWave = kTileH / 4;

template <int C> struct CasTile
{
    static constexpr int in_stride = (kTileW + 2) * C;                              // floats per staged row (halo included)
    static constexpr int in_dwords = ((kTileW + 2) * C + 3 + 3) / 4;                // aligned dwords that can cover one staged row
    static constexpr int out_stride = (kTileW * C + 3 + 3) / 4 * 4;                 // bytes per output row (alignment offset + row)
    static constexpr int out_dwords = out_stride / 4;
};

using namespace ffx;                       // unit_of, sat, to_byte, cas_channel: the arithmetic, shared with cas_gray.hip

template <int C>
__global__ __launch_bounds__(256)
void k_cas(const uint8_t* __restrict__ src, long long src_step, int rows, int cols, uint8_t* __restrict__ dst, long long dst_step, float peak)
{
    using T = CasTile<C>;
    __shared__ float tin[(kTileH + 2) * T::in_stride];
    __shared__ __attribute__((aligned(4))) uint8_t tout[kTileH * T::out_stride];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kTileW;
    const long long row_bytes = (long long)cols * C;
    const int s0 = (x0 - 1) * C;                                 // byte of the row where the staged segment starts (may be -C)
    const int seg = (kTileW + 2) * C;

    for (int y0 = blockIdx.y * kTileH; y0 < rows; y0 += gridDim.y * kTileH)
    {
        // ---- load: zero outside the frame (edge tiles only), then the frame's bytes as floats
        const bool edge = x0 == 0 || (long long)(x0 + kTileW + 1) * C > row_bytes || y0 == 0 || y0 + kTileH >= rows;
        if (edge)
        {
            for (int k = tid; k < (kTileH + 2) * T::in_stride; k += 256) tin[k] = 0.0f;
            __syncthreads();
        }
        const long long v0 = s0 < 0 ? 0 : s0;
        const long long v1 = (long long)s0 + seg < row_bytes ? (long long)s0 + seg : row_bytes;
        for (int k = tid; k < (kTileH + 2) * T::in_dwords; k += 256)
        {
            const int tr = k / T::in_dwords, kd = k - tr * T::in_dwords;
            const int y = y0 - 1 + tr;
            if (y < 0 || y >= rows) continue;
            const uintptr_t rowp = (uintptr_t)(src + (long long)y * src_step);
            const uintptr_t a0 = (rowp + v0) & ~(uintptr_t)3;
            const uintptr_t q = a0 + 4 * (uintptr_t)kd;
            if (q >= rowp + v1) continue;                        // past the last dword that holds a byte of the segment
            const uint32_t word = *(const uint32_t*)q;
            float* trow = tin + tr * T::in_stride;
#pragma unroll
            for (int b = 0; b < 4; b++)
            {
                const long long off = (long long)(q + b - rowp);   // byte of the frame row
                if (off < v0 || off >= v1) continue;
                const int pos = (int)(off - s0);                 // byte of the staged segment
                if (C == 4 && (pos & 3) == 3) continue;           // the 4th channel is written as 255, never read
                trow[pos] = unit_of((float)((word >> (8 * b)) & 0xffu));
            }
        }
        __syncthreads();

        // ---- compute: one column per lane, a sliding 3-row window down this wave's rows
        const int ty0 = wave * kRowsPerWave;
        float win[3][3][3];                                      // [row][pixel left / centre / right][channel]
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int p = 0; p < 3; p++)
#pragma unroll
                for (int c = 0; c < 3; c++) win[r][p][c] = tin[(ty0 + r) * T::in_stride + (lane + p) * C + c];
#pragma unroll
        for (int j = 0; j < kRowsPerWave; j++)
        {
            const int ty = ty0 + j;
#pragma unroll
            for (int p = 0; p < 3; p++)
#pragma unroll
                for (int c = 0; c < 3; c++) win[2][p][c] = tin[(ty + 2) * T::in_stride + (lane + p) * C + c];
            const int y = y0 + ty;
            if (y < rows)
            {
                const uintptr_t d0 = (uintptr_t)(dst + (long long)y * dst_step + (long long)x0 * C);
                uint8_t* orow = tout + ty * T::out_stride + (int)(d0 & 3) + lane * C;
#pragma unroll
                for (int c = 0; c < 3; c++)
                {
                    const float v = cas_channel(win[0][0][c], win[0][1][c], win[0][2][c], win[1][0][c], win[1][1][c], win[1][2][c],
                                                win[2][0][c], win[2][1][c], win[2][2][c], peak);
                    orow[c] = (uint8_t)to_byte(v);
                }
                if (C == 4) orow[3] = 255;
            }
#pragma unroll
            for (int p = 0; p < 3; p++)
#pragma unroll
                for (int c = 0; c < 3; c++) { win[0][p][c] = win[1][p][c]; win[1][p][c] = win[2][p][c]; }
        }
        __syncthreads();

        // ---- store: aligned dwords inside [x0 * C, min(x0 + 64, cols) * C) of each row, single bytes at the two ends
        const long long e0 = (long long)x0 * C;
        const long long e1 = (long long)(x0 + kTileW) * C < row_bytes ? (long long)(x0 + kTileW) * C : row_bytes;
        for (int k = tid; k < kTileH * T::out_dwords; k += 256)
        {
            const int ty = k / T::out_dwords, kd = k - ty * T::out_dwords;
            const int y = y0 + ty;
            if (y >= rows) continue;
            const uintptr_t rowp = (uintptr_t)(dst + (long long)y * dst_step);
            const uintptr_t d0 = rowp + e0, d1 = rowp + e1;
            const uintptr_t base = d0 & ~(uintptr_t)3;
            const uintptr_t q = base + 4 * (uintptr_t)kd;
            if (q >= d1) continue;
            const uint8_t* orow = tout + ty * T::out_stride + 4 * kd;
            if (q >= d0 && q + 4 <= d1)
                *(uint32_t*)q = *(const uint32_t*)orow;
            else
            {
#pragma unroll
                for (int b = 0; b < 4; b++)
                    if (q + b >= d0 && q + b < d1) *(uint8_t*)(q + b) = orow[b];
            }
        }
        __syncthreads();                                         // the tiles are reused by the next row of tiles
    }
}

} // namespace

extern "C" {

int lvk_hip_cas_const(float sharpness, float* peak)
{
    if (!peak || std::isnan(sharpness)) return LVK_HIP_ERR_ARG;
    // CasSetup: ALerpF1(8, 5, s) = 5 s + ((-8) s + 8) and -ARcpF1 of it, each float operation rounded on its own (-ffp-contract=off)
    const float s = sharpness < 0.0f ? 0.0f : sharpness > 1.0f ? 1.0f : sharpness;
    const float lerp = 5.0f * s + (-8.0f * s + 8.0f);
    *peak = -(1.0f / lerp);
    return LVK_HIP_OK;
}

int lvk_hip_cas(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, int format, void* d_dst, int dst_step, float sharpness)
{
    LVK_HIP_ENTRY(ctx);
    const int ch = lvk_format_channels(format);
    if (ch != 3 && ch != 4) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_cas: packed BGR / RGB / YUV / BGRA / RGBA frames only");
    if (!(sharpness >= 0.0f && sharpness <= 1.0f)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_cas: sharpness must lie in [0, 1] (CASFilter.cpp)");
    LVK_HIP_REQUIRE(ctx, d_src && d_dst && rows > 0 && cols > 0);
    const long long row_bytes = (long long)cols * ch;
    LVK_HIP_REQUIRE(ctx, (long long)src_step >= row_bytes && (long long)dst_step >= row_bytes);
    // CAS reads its neighbours: a destination that overlaps the source (in place included) would race
    if (lvk_pitched_overlap(d_src, src_step, rows, row_bytes, d_dst, dst_step, rows, row_bytes)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_cas: the source and destination overlap");
    float peak = 0.0f;
    lvk_hip_cas_const(sharpness, &peak);

    const unsigned gx = (unsigned)((cols + kTileW - 1) / kTileW);
    const unsigned gy = (unsigned)std::min<long long>(((long long)rows + kTileH - 1) / kTileH, 65535);
    if (ch == 3)
        hipLaunchKernelGGL(k_cas<3>, dim3(gx, gy), dim3(256), 0, ctx->stream, (const uint8_t*)d_src, (long long)src_step, rows, cols,
                           (uint8_t*)d_dst, (long long)dst_step, peak);
    else
        hipLaunchKernelGGL(k_cas<4>, dim3(gx, gy), dim3(256), 0, ctx->stream, (const uint8_t*)d_src, (long long)src_step, rows, cols,
                           (uint8_t*)d_dst, (long long)dst_step, peak);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

} // extern "C"
