// The FSR filter's EASU pass (fsr.hip) on ONE-channel frames (8UC1, VideoFrame::GRAY) for gfx950: the kernels behind lvk_hip_fsr_easu_gray.
//
// The plugin runs FSR as an RGBA effect, so there is no one-channel program to copy.  DEFINITION: channel 0 of the
// three-channel specification (tests/np_fsr.py) on (g, g, g), which is the same for BGR, RGB and YUV.  The geometry is that of
// lvk_hip_fsr_geometry: a crop region, taps clamped to the frame, any output size.  The direction / length analysis and the tap weights are the
// functions of fsr_core.hpp that k_fsr_easu<C, kStaged> calls; here they feed one accumulator and one de-ringing clamp instead of three.  The luma
// of a grey texel, 0.5 v + (0.5 v + v) in binary32, is 2 v exactly for all 256 bytes (tests/test_ffx_gray_spec.py pins it) and is formed as v + v.
//
// One kernel, k_fsr_easu_gray<kStaged>, on the tile walk of fsr_core.hpp with float texels; what it adds is that all 64 lanes of a wave run the row
// loop (for the shuffles of store_row) and the row store.  The two tap paths:
//   staged   the tile's source footprint is read once into LDS as one float per texel (the luma is one addition per tap: staging it too would
//            double the LDS reads and halve the footprints that fit).  A texel is 4 bytes, not 16, so four times the footprint fits the same
//            40 KiB and most downscales stay staged.
//   direct   each tap reads its byte from the frame (footprints beyond the stage).
// Output: the four lanes whose bytes share an aligned dword of the destination row hand them to the first of the four (wave shuffles), which
// stores the dword; lanes whose dword is cut by the tile's or the row's end store their byte.  No byte outside out_cols of a row is written.
#include "lvk_hip_internal.hpp"
#include "fsr_core.hpp"

#include <algorithm>
#include <cstdint>

namespace {

using namespace ffx;

struct EasuGrayArgs
{
    const uint8_t* src;
    long long src_step;
    uint8_t* dst;
    long long dst_step;
};

// FsrEasuF with one channel, from the 12 taps t[dy + 1][dx + 1] (dx, dy in -1 .. 2; the four corners are not used) and the fraction of pp
__device__ __forceinline__ float easu_gray(const float (&t)[4][4], float ppx, float ppy)
{
    const float b = t[0][1], c = t[0][2], e = t[1][0], f = t[1][1], g = t[1][2], h = t[1][3];
    const float i = t[2][0], j = t[2][1], k = t[2][2], l = t[2][3], n = t[3][1], o = t[3][2];
    const EasuLobe lobe = easu_analyse(b + b, c + c, e + e, f + f, g + g, h + h, i + i, j + j, k + k, l + l, n + n, o + o, ppx, ppy);
    float ac = 0.0f, aw = 0.0f;
    easu_taps(t, [&](float ox, float oy, float v) {
        const float w = easu_weight(ox, oy, ppx, ppy, lobe);
        ac = ac + v * w;
        aw = aw + w;
    });
    const float inv = 1.0f / aw;                       // correctly rounded (ARcpF1 on OpenGL)
    const float mn = __builtin_fminf(__builtin_fminf(__builtin_fminf(f, g), j), k);
    const float mx = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(f, g), j), k);
    return __builtin_fminf(mx, __builtin_fmaxf(mn, ac * inv));
}

// One output row of a wave: lane `lane` holds the byte of column x (live: x < out_cols).  Called by all 64 lanes.
__device__ __forceinline__ void store_row(const EasuGrayArgs& a, int out_cols, int x, int y, int lane, bool live, uint32_t byte)
{
    uint8_t* p = a.dst + (long long)y * a.dst_step + x;
    const int al = (int)(reinterpret_cast<uintptr_t>(p) & 3u);
    const uint32_t b1 = __shfl_down(byte, 1), b2 = __shfl_down(byte, 2), b3 = __shfl_down(byte, 3);
    // the dword that holds this lane's byte starts at lane - al, column x - al: whole when its four bytes are live lanes of this wave
    const bool whole = lane - al >= 0 && lane - al + 3 < 64 && x - al + 3 < out_cols;
    if (!live) return;
    if (!whole) *p = (uint8_t)byte;
    else if (al == 0) *reinterpret_cast<uint32_t*>(p) = byte | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

template <bool kStaged>
__global__ __launch_bounds__(256)
void k_fsr_easu_gray(EasuGrayArgs a, FsrGeo g)
{
    __shared__ float stage[kStaged ? kStageTexels<float> : 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kTileW;
    const int x = x0 + lane;
    const bool live = x < g.out_cols;
    // (a lane beyond the row's end computes the row's last column, so that it stays inside the footprint and takes part in the shuffles)
    const EasuCol col = easu_col(g, x0, min(x, g.out_cols - 1));
    const auto fetch = [&](int sx, int sy) { return unit_of((float)a.src[(long long)sy * a.src_step + sx]); };

    for (int y0 = blockIdx.y * kTileH; y0 < g.out_rows; y0 += gridDim.y * kTileH)
    {
        const int fy0 = kStaged ? easu_stage_fill(stage, g, col, y0, tid, fetch) : 0;
#pragma unroll 1
        for (int j = 0; j < kRowsPerWave; j++)
        {
            const int y = y0 + wave * kRowsPerWave + j;
            if (y >= g.out_rows) break;                             // (wave-uniform)
            float t[4][4];
            const float ppy = easu_gather<kStaged>(t, stage, g, col, fy0, y, fetch);
            store_row(a, g.out_cols, x, y, lane, live, to_byte(easu_gray(t, col.ppx, ppy)));
        }
        if (kStaged) __syncthreads();                               // the stage is reused by the next row of tiles
    }
}

} // namespace

extern "C" {

int lvk_hip_fsr_easu_gray_path(int rw, int rh, int out_rows, int out_cols)
{
    return fsr_stage_fits(rw, rh, out_rows, out_cols, kStageTexels<float>);
}

int lvk_hip_fsr_easu_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, const int region_xywh[4], void* d_dst,
                          int dst_step, int out_rows, int out_cols)
{
    LVK_HIP_ENTRY(ctx);
    LVK_HIP_REQUIRE(ctx, d_src && d_dst && region_xywh && rows > 0 && cols > 0 && out_rows > 0 && out_cols > 0);
    if (!fsr_region_ok(region_xywh, rows, cols))
        return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_fsr_easu_gray: the region must be a non-empty rectangle inside the frame");
    LVK_HIP_REQUIRE(ctx, src_step >= cols && dst_step >= out_cols);
    if (lvk_pitched_overlap(d_src, src_step, rows, cols, d_dst, dst_step, out_rows, out_cols)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_fsr_easu_gray: the source and destination overlap");

    const EasuGrayArgs a{(const uint8_t*)d_src, (long long)src_step, (uint8_t*)d_dst, (long long)dst_step};
    const FsrGeo geo = fsr_geo(rows, cols, region_xywh, out_rows, out_cols);
    const bool staged = lvk_hip_fsr_easu_gray_path(region_xywh[2], region_xywh[3], out_rows, out_cols) == 0;
    if (staged) hipLaunchKernelGGL((k_fsr_easu_gray<true>), fsr_grid(geo), dim3(256), 0, ctx->stream, a, geo);
    else hipLaunchKernelGGL((k_fsr_easu_gray<false>), fsr_grid(geo), dim3(256), 0, ctx->stream, a, geo);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

} // extern "C"
