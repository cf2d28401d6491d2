// The FSR 1 EASU pass on the PLANES of an OBS video format (lvk_hip_fsr_yuv420: fsr_420.hip; lvk_hip_fsr_obs: fsr_obs.hip): the one
// kernel body both units instantiate, its launch, and what the two entries check alike.  The output planes are byte for byte those of
//   ingest -> lvk_hip_fsr_easu(format = YUV) -> egress
// so the kernel stands on what k_fsr_easu<3, .> of fsr.hip stands on (the tile walk and easu of fsr_core.hpp, on texels (Y, U, V, luma), luma =
// 0.5 V + (0.5 Y + U)) with the ingest in front of its taps and the egress behind its pixels:
//   Src    px(sx, sy): the packed pixel 0x00VVUUYY the ingest writes at (sx, sy) of the frame, formed from the planes -- the chroma UP-SAMPLED by the
//          ingest's closed forms at FRAME coordinates, so a region at an odd origin reads the other chroma phase.  sx, sy are clamped into the frame
//          first (the point sampler's clamp), then the chroma phase is taken; the up-sampling clamps its own far sample (the edge replicated).
//   staged the tile's source footprint goes through Src once into LDS as float4: the ONE place the planes are read; a texel is converted once
//   direct the taps read a packed 8UC3 frame (PackedYuv: the pooled frame the ingest kernels made) with clamped indices
//   Out    the sinks take four horizontally adjacent pixels (obs_sinks.hpp), the 4:2:0 stores four columns of a row pair (yuv420_core.hpp), while a
//          thread of the tile computes a COLUMN of four rows.  So every thread puts its four pixels as 0x00VVUUYY into an LDS out-tile of 16 x 64
//          words, and after a barrier the threads read it back in the output's shape: the quad mean (sum + 2) >> 2 of 4:2:0 and the pair sum halved
//          half-to-even of 4:2:2 are taken there, on the scaled full-resolution chroma, as the egress takes them.  Both tile sides are even and the
//          width a multiple of 4: no quad, pair or group of four straddles two tiles.  The out-tile aliases the first 4 KiB of the stage (a barrier
//          after the last tap), so the stage keeps the 40 KiB of every EASU kernel and four blocks fit a CU.
// No load touches a byte outside the used bytes of a plane row, and no store one outside those of an output row.
#pragma once

#include "lvk_hip_internal.hpp"
#include "fsr_core.hpp"
#include "yuv420_core.hpp"

#include <algorithm>

namespace {

using namespace ffx;

constexpr int kFsrOutWords = kTileW * kTileH;          // the out-tile: 4 KiB, inside the stage

// (Y, U, V, luma) of a packed pixel 0x00VVUUYY: texel() of fsr.hip with r, g, b = bytes 0, 1, 2
__device__ __forceinline__ float4 yuv_texel(uint32_t px)
{
    const float r = unit_of((float)(px & 0xffu)), g = unit_of((float)((px >> 8) & 0xffu)), b = unit_of((float)((px >> 16) & 0xffu));
    return make_float4(r, g, b, b * 0.5f + (r * 0.5f + g));
}

// a packed 8UC3 YUV frame (the direct path's source)
struct PackedYuv
{
    const uint8_t* p; int step;
    __device__ __forceinline__ uint32_t px(int sx, int sy) const
    {
        const uint8_t* q = p + (size_t)sy * step + 3 * (size_t)sx;
        return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    }
};

// The 4:2:0 planes as the ingest reads them (yuv420_core.hpp: t = 3 C[c] + C[f] along the row, up_v down the column, f and g clamped to the plane)
template <bool NV12>
struct Src420
{
    yuv420::Planes in; int cr, cc;         // the chroma plane's rows and columns
    __device__ __forceinline__ uint32_t px(int sx, int sy) const
    {
        constexpr int PIX = NV12 ? 2 : 1;
        const int c = sx >> 1, f = min(max((sx & 1) ? c + 1 : c - 1, 0), cc - 1);
        const int k = sy >> 1, g = min(max((sy & 1) ? k + 1 : k - 1, 0), cr - 1);
        const uint8_t* uk = in.u + (size_t)k * in.us;
        const uint8_t* ug = in.u + (size_t)g * in.us;
        const uint8_t* vk = NV12 ? uk + 1 : in.v + (size_t)k * in.vs;
        const uint8_t* vg = NV12 ? ug + 1 : in.v + (size_t)g * in.vs;
        const uint32_t y = in.y[(size_t)sy * in.ys + sx];
        const uint32_t u = (uint32_t)yuv420::up_v(3 * uk[c * PIX] + uk[f * PIX], 3 * ug[c * PIX] + ug[f * PIX]);
        const uint32_t v = (uint32_t)yuv420::up_v(3 * vk[c * PIX] + vk[f * PIX], 3 * vg[c * PIX] + vg[f * PIX]);
        return y | (u << 8) | (v << 16);
    }
};

// the output planes of a 4:2:0 frame: thread t < 128 of the block stores the four columns 4 (t & 15) .. of the row pair t >> 4 of the tile
template <bool NV12>
struct Out420
{
    yuv420::PlanesOut out; int flags;      // yuv420::access_flags
    __device__ __forceinline__ void store_tile(const float* tile, int x0, int y0, int out_rows, int out_cols, int tid) const
    {
        const int k = tid >> 4, x = x0 + 4 * (tid & 15), ya = y0 + 2 * k;
        if (tid >= 128 || x >= out_cols || ya >= out_rows) return;
        const bool half = x + 4 > out_cols;                 // the row's last two columns
        uint32_t o[2][4];
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int p = 0; p < 4; p++) o[r][p] = as_u(tile[(2 * k + r) * kTileW + 4 * (tid & 15) + p]);
        yuv420::store_luma4(out.y + (size_t)ya * out.ys + x, o[0], half, flags);
        yuv420::store_luma4(out.y + (size_t)(ya + 1) * out.ys + x, o[1], half, flags);
        uint32_t u[2], v[2];                                // INTER_AREA 0.5 x 0.5 of each 2 x 2 quad of output pixels
#pragma unroll
        for (int q = 0; q < 2; q++)
        {
            const uint32_t a = o[0][2 * q], b = o[0][2 * q + 1], c = o[1][2 * q], d = o[1][2 * q + 1];
            u[q] = (((a >> 8) & 0xffu) + ((b >> 8) & 0xffu) + ((c >> 8) & 0xffu) + ((d >> 8) & 0xffu) + 2) >> 2;
            v[q] = (((a >> 16) & 0xffu) + ((b >> 16) & 0xffu) + ((c >> 16) & 0xffu) + ((d >> 16) & 0xffu) + 2) >> 2;
        }
        yuv420::store_chroma2<NV12>(out, ya >> 1, x >> 1, u, v, half, flags);
    }
};

template <class Src, class Out, bool kStaged>
__global__ __launch_bounds__(256)
void k_fsr_planes(Src src, Out out, FsrGeo a)
{
    __shared__ float4 stage[kStaged ? kStageTexels<float4> : kFsrOutWords / 4];
    float* tile = reinterpret_cast<float*>(stage);                 // the out-tile: words carried as floats, bits untouched

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kTileW;
    const int x = x0 + lane;
    const EasuCol col = easu_col(a, x0, x);
    const auto fetch = [&](int sx, int sy) { return yuv_texel(src.px(sx, sy)); };

    for (int y0 = blockIdx.y * kTileH; y0 < a.out_rows; y0 += gridDim.y * kTileH)
    {
        const int fy0 = kStaged ? easu_stage_fill(stage, a, col, y0, tid, fetch) : 0;
        uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;                    // the thread's column of four pixels
        if (x < a.out_cols)
        {
#pragma unroll 1
            for (int j = 0; j < kRowsPerWave; j++)
            {
                const int y = y0 + wave * kRowsPerWave + j;
                if (y >= a.out_rows) break;
                float4 t[4][4];
                const float ppy = easu_gather<kStaged>(t, stage, a, col, fy0, y, fetch);
                const float3 pix = easu(t, col.ppx, ppy);
                const uint32_t w = to_byte(pix.x) | (to_byte(pix.y) << 8) | (to_byte(pix.z) << 16);
                o0 = j == 0 ? w : o0; o1 = j == 1 ? w : o1; o2 = j == 2 ? w : o2; o3 = j == 3 ? w : o3;      // no indexed array: no scratch
            }
        }
        if (kStaged) __syncthreads();                               // every tap is read: the out-tile takes the stage's first words
        float* out_col = tile + wave * kRowsPerWave * kTileW + lane;
        out_col[0] = as_f(o0); out_col[kTileW] = as_f(o1); out_col[2 * kTileW] = as_f(o2); out_col[3 * kTileW] = as_f(o3);
        __syncthreads();
        out.store_tile(tile, x0, y0, a.out_rows, a.out_cols, tid);
        __syncthreads();                                            // the tile and the stage are reused by the next row of tiles
    }
}

template <class Src, class Out, bool kStaged>
int launch_fsr_planes(lvk_hip_ctx* ctx, const Src& src, const Out& out, const FsrGeo& a)
{
    hipLaunchKernelGGL((k_fsr_planes<Src, Out, kStaged>), fsr_grid(a), dim3(256), 0, ctx->stream, src, out, a);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// the packed frame of the direct route: its pitch (rows on a dword, where the ingest kernels take their wide stores)
inline int fsr_packed_step(int cols) { return (3 * cols + 3) & ~3; }

} // namespace
