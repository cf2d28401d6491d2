// The OBS plugin's FSR filter (FSRFilter / FSREffect: the FidelityFX FSR 1 EASU pass of fsr.effect, point-sampled gathers, no RCAS) on
// the MI355X, out of place from a crop region of a packed 3- or 4-channel frame to an output of any size.  Specification: tests/np_fsr.py
// and DESIGN.md section 16.
//
// One kernel, k_fsr_easu<C, kStaged>, on the context's stream.  A block of 256 threads owns a 64 x 16 pixel output tile; lane l of wave w
// computes column l of rows 4w .. 4w + 3.  The tile walk (which texel a tap is, the stage fill, the 12-tap gather) and the pixel function are
// fsr_core.hpp's; this unit adds the texel of a packed pixel, the skip of the lanes beyond the row's end and the pixel store.  Two ways to
// fetch a tap, chosen per launch by the host from the scale:
//   staged   the tile's source footprint (its fp range plus the -1 .. 2 taps) is read once into LDS as float4 (r, g, b, luma): each texel
//            is converted and its luma computed once, not once per tap.  Used when the largest footprint of the launch fits the stage.
//   direct   each tap reads its bytes from the frame and computes its luma (downscales whose footprint does not fit).
// The arithmetic is the specification's, unfused, with the FidelityFX bit tricks and a correctly rounded 1 / aW.  Output bytes are
// stored one channel at a time (a whole dword for 4-channel pixels at an aligned address): no byte outside out_cols * C of a row is written.
#include "lvk_hip_internal.hpp"
#include "fsr_core.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

using namespace ffx;                       // the tile and its walk, FsrEasuF on float4 texels, the byte conversions, the host's prelude (fsr_core.hpp)

struct EasuArgs
{
    const uint8_t* src;
    long long src_step;
    uint8_t* dst;
    long long dst_step;
    int ri, bi;                            // byte of the shader's r and b (g is byte 1)
};

// (r, g, b, luma) of the texel at byte p of the frame
__device__ __forceinline__ float4 texel(const uint8_t* p, int ri, int bi)
{
    const float r = unit_of((float)p[ri]), g = unit_of((float)p[1]), b = unit_of((float)p[bi]);
    return make_float4(r, g, b, b * 0.5f + (r * 0.5f + g));
}

template <int C>
__device__ __forceinline__ void store_pixel(const EasuArgs& a, int x, int y, float3 pix)
{
    uint8_t* p = a.dst + (long long)y * a.dst_step + (long long)x * C;
    const uint32_t r = to_byte(pix.x), g = to_byte(pix.y), b = to_byte(pix.z);
    if (C == 4 && ((uintptr_t)p & 3) == 0)
    {
        *(uint32_t*)p = (r << (8 * a.ri)) | (g << 8) | (b << (8 * a.bi)) | 0xff000000u;
        return;
    }
    p[a.ri] = (uint8_t)r;
    p[1] = (uint8_t)g;
    p[a.bi] = (uint8_t)b;
    if (C == 4) p[3] = 255;
}

template <int C, bool kStaged>
__global__ __launch_bounds__(256)
void k_fsr_easu(EasuArgs a, FsrGeo g)
{
    __shared__ float4 stage[kStaged ? kStageTexels<float4> : 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kTileW;
    const int x = x0 + lane;
    const EasuCol col = easu_col(g, x0, x);
    const auto fetch = [&](int sx, int sy) { return texel(a.src + (long long)sy * a.src_step + (long long)sx * C, a.ri, a.bi); };

    for (int y0 = blockIdx.y * kTileH; y0 < g.out_rows; y0 += gridDim.y * kTileH)
    {
        const int fy0 = kStaged ? easu_stage_fill(stage, g, col, y0, tid, fetch) : 0;
        if (x < g.out_cols)
        {
#pragma unroll 1
            for (int j = 0; j < kRowsPerWave; j++)
            {
                const int y = y0 + wave * kRowsPerWave + j;
                if (y >= g.out_rows) break;
                float4 t[4][4];
                const float ppy = easu_gather<kStaged>(t, stage, g, col, fy0, y, fetch);
                store_pixel<C>(a, x, y, easu(t, col.ppx, ppy));
            }
        }
        if (kStaged) __syncthreads();                               // the stage is reused by the next row of tiles
    }
}

// cvRound of a float32 (round half to even), saturating far beyond the output cap
int cv_round(float v) { return v >= 1.0e9f ? 1000000000 : (int)std::nearbyint(v); }

} // namespace

extern "C" {

int lvk_hip_fsr_easu_const(int rw, int rh, int W, int H, int ow, int oh, float con[16])
{
    if (!con || rw <= 0 || rh <= 0 || W <= 0 || H <= 0 || ow <= 0 || oh <= 0) return LVK_HIP_ERR_ARG;
    // FsrEasuCon on the CPU, each float operation rounded on its own (-ffp-contract=off); rcp is 1 / x
    const float frw = (float)rw, frh = (float)rh, rW = 1.0f / (float)W, rH = 1.0f / (float)H, row = 1.0f / (float)ow, roh = 1.0f / (float)oh;
    const float v[16] = {frw * row, frh * roh, (0.5f * frw) * row - 0.5f, (0.5f * frh) * roh - 0.5f,
                         rW, rH, 1.0f * rW, -1.0f * rH,
                         -1.0f * rW, 2.0f * rH, 1.0f * rW, 2.0f * rH,
                         0.0f * rW, 4.0f * rH, 0.0f, 0.0f};
    std::copy(v, v + 16, con);
    return LVK_HIP_OK;
}

int lvk_hip_fsr_easu_path(int rw, int rh, int out_rows, int out_cols)
{
    return fsr_stage_fits(rw, rh, out_rows, out_cols, kStageTexels<float4>);
}

int lvk_hip_fsr_geometry(int rows, int cols, int out_rows, int out_cols, float multiplier, int maintain_aspect_ratio, const int crop_ltrb[4],
                         int region_xywh[4], int out_rows_cols[2], int* skip)
{
    if (rows <= 0 || cols <= 0 || out_rows < 0 || out_cols < 0 || !crop_ltrb || !region_xywh || !out_rows_cols || !skip) return LVK_HIP_ERR_ARG;
    for (int k = 0; k < 4; k++)
        if (crop_ltrb[k] < 0 || crop_ltrb[k] > 4096) return LVK_HIP_ERR_ARG;
    const bool by_multiplier = out_rows == 0 && out_cols == 0;
    if (by_multiplier && !(multiplier > 0.0f && std::isfinite(multiplier))) return LVK_HIP_ERR_ARG;
    // FSRFilter::tick: the output size ...
    int ow = out_cols, oh = out_rows;
    if (by_multiplier) { ow = cv_round((float)cols * multiplier); oh = cv_round((float)rows * multiplier); }
    // ... the crop region ...
    const int l = crop_ltrb[0], t = crop_ltrb[1], r = crop_ltrb[2], b = crop_ltrb[3];
    int rx = 0, ry = 0, rw = cols, rh = rows;
    if (l + r < cols && t + b < rows) { rx = l; ry = t; rw = cols - r - l; rh = rows - b - t; }
    // ... the aspect-ratio fit and the 4096 cap
    if (maintain_aspect_ratio && (long long)rw * rh != 0)
    {
        const float s = std::min((float)ow / (float)rw, (float)oh / (float)rh);
        ow = cv_round((float)rw * s);
        oh = cv_round((float)rh * s);
    }
    ow = std::min(ow, 4096);
    oh = std::min(oh, 4096);
    region_xywh[0] = rx; region_xywh[1] = ry; region_xywh[2] = rw; region_xywh[3] = rh;
    out_rows_cols[0] = oh; out_rows_cols[1] = ow;
    // OBSEffect::is_renderable + FSREffect::should_skip (the region is inside the frame and not empty by construction)
    *skip = (ow <= 0 || oh <= 0 || (ow == cols && oh == rows && rw == cols && rh == rows)) ? 1 : 0;
    return LVK_HIP_OK;
}

int lvk_hip_fsr_easu(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, int format, const int region_xywh[4], void* d_dst,
                     int dst_step, int out_rows, int out_cols)
{
    LVK_HIP_ENTRY(ctx);
    const int ch = lvk_format_channels(format);
    if (ch != 3 && ch != 4) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_fsr_easu: packed BGR / RGB / YUV / BGRA / RGBA frames only");
    LVK_HIP_REQUIRE(ctx, d_src && d_dst && region_xywh && rows > 0 && cols > 0 && out_rows > 0 && out_cols > 0);
    if (!fsr_region_ok(region_xywh, rows, cols))
        return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_fsr_easu: the region must be a non-empty rectangle inside the frame");
    const long long src_row = (long long)cols * ch, dst_row = (long long)out_cols * ch;
    LVK_HIP_REQUIRE(ctx, (long long)src_step >= src_row && (long long)dst_step >= dst_row);
    if (lvk_pitched_overlap(d_src, src_step, rows, src_row, d_dst, dst_step, out_rows, dst_row)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_fsr_easu: the source and destination overlap");

    const bool bgr = format == LVK_FORMAT_BGR || format == LVK_FORMAT_BGRA;
    const EasuArgs a{(const uint8_t*)d_src, (long long)src_step, (uint8_t*)d_dst, (long long)dst_step, bgr ? 2 : 0, bgr ? 0 : 2};
    const FsrGeo geo = fsr_geo(rows, cols, region_xywh, out_rows, out_cols);
    const bool staged = lvk_hip_fsr_easu_path(region_xywh[2], region_xywh[3], out_rows, out_cols) == 0;
    const dim3 grid = fsr_grid(geo);
    if (ch == 3)
    {
        if (staged) hipLaunchKernelGGL((k_fsr_easu<3, true>), grid, dim3(256), 0, ctx->stream, a, geo);
        else hipLaunchKernelGGL((k_fsr_easu<3, false>), grid, dim3(256), 0, ctx->stream, a, geo);
    }
    else
    {
        if (staged) hipLaunchKernelGGL((k_fsr_easu<4, true>), grid, dim3(256), 0, ctx->stream, a, geo);
        else hipLaunchKernelGGL((k_fsr_easu<4, false>), grid, dim3(256), 0, ctx->stream, a, geo);
    }
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

} // extern "C"
