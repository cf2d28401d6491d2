// lvk::DeblockingFilter (Filters/DeblockingFilter.{hpp,cpp}) on the MI355X: the adaptive blend of a median-smoothed frame into the original, in
// place on a packed frame of one (8UC1, GRAY), three (8UC3, BGR / RGB / YUV) or four (8UC4, BGRA / RGBA) bytes per pixel.
// Specification: tests/np_deblock.py, tests/np_deblock_px.py and DESIGN.md sections 13 and 23.  What this unit shares with deblock_420.hip (the
// same filter on I420 / NV12 planes) -- the handle, the per-pixel arithmetic, the downscale's body, the geometry -- is in deblock_core.hpp.
//
// The reference's filter is made of channel-agnostic OpenCV calls (Filters/DeblockingFilter.cpp:48-110: cv::resize, cv::medianBlur, reformatTo(GRAY),
// cv::blendLinear), so every pixel size is the reference's own: one operation order and one set of rounding rules, per channel.  The ALPHA byte of a
// four-channel frame is a channel like the others -- downscaled, median-filtered, up-sampled and blended under the same `keep` map --, because that is
// what those calls do to an 8UC4 UMat.  This differs on purpose from lvk_hip_sharpen_c4 and the four-channel remap, whose alpha had no reference program
// and was defined here.
//
// Four kernels per apply with the bytes per pixel (BPP = 1 / 3 / 4) as a template parameter, all on the context's stream, nothing synchronises:
//   k_deblock_stats    one wave per macroblock: exact integer block mean of the grey, mean absolute deviation from it (second pass over the same,
//                      cache-resident bytes), keep_block = float(min(grid, L) * (1.0 / L)).  The grey is the byte itself for GRAY and byte 0 of a YUV
//                      frame, else the fixed-point BT.601 of the colour bytes (the format selects which byte is blue; alpha ignored).  Four channels:
//                      one dword per pixel; three: three byte loads; GRAY: one dword per four pixels where the block rows are dword-aligned (block
//                      size, base and pitch multiples of 4), else bytes.
//   k_deblock_down     INTER_AREA of the region by 1 / filter_scaling, one thread per output pixel and BPP sums: integer box rule at integer scales
//                      (partial cells (float)sum / count), area tables in table order else.
//   k_deblock_median   exact per-channel median of the k x k window (BORDER_REPLICATE) on the small frame: LDS tile with a replicated apron, a radix
//                      selection (8 counting passes, one counter set per channel) over a register window for k = 3 / 5, over the tile for larger k.
//                      The tile holds one PIXEL per element: a dword (the channels packed) for three- and four-channel frames, ONE BYTE for GRAY --
//                      a GRAY tile is a quarter of the size and is read with byte loads; the register window holds one pixel per register either way.
//   k_deblock_blend    rebuilds `smooth` (8U bilinear from the median frame) and `keep` (float bilinear from keep_block) per pixel and writes the
//                      blend in place; the full-size smooth / keep / deblock frames of the reference are never materialised.  Three and four
//                      channels: one thread per pixel, the four taps of `smooth` and the frame pixel as one pixel load each (a dword for four
//                      channels, three bytes for three).  GRAY (k_deblock_blend_gray): one thread per group of four pixels; the groups of a row
//                      start at the dword boundary at or below the row's first byte (so every row is aligned whatever the base and the pitch are),
//                      a group that lies inside the region is one dword load and one dword store, the first and the last group of a row go byte by
//                      byte over the pixels they hold.
// draw_influence (8UC3 only, as in the reference) is the three-channel blend with a constant colour for `smooth` and the keep_block of the last apply.
// No load or store touches a byte outside the rw * BPP bytes of a region row, and only the region is written.  Three-channel pixels are moved byte by
// byte and need no alignment; a four-channel frame is dword-aligned (apply refuses others).
#include "deblock_core.hpp"

using namespace deblock;

namespace {

constexpr int kMedTile = 16;              // median: 16 x 16 outputs per block
constexpr int kMedLdsMaxK = 113;          // (16 + k - 1)^2 packed pixels fit 64 KiB of LDS up to this k; larger k read global memory

// The grey of the block statistics.  GRAY: the byte itself.  Else RGB2Gray<uchar> of the colour bytes; blue_shift: the bit position of the blue
// byte (0: BGR / BGRA, 16: RGB / RGBA), alpha ignored; negative (three-channel YUV): byte 0.  blue_shift is a kernel argument, uniform over the grid.
template <int BPP>
__device__ __forceinline__ int gray_of(uint32_t v, int blue_shift)
{
    if (BPP == 1 || (BPP == 3 && blue_shift < 0)) return (int)(v & 255u);
    const int b = (int)((v >> blue_shift) & 255u), g = (int)((v >> 8) & 255u), r = (int)((v >> (16 - blue_shift)) & 255u);
    return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15;
}

// f(grey) for every pixel of one macroblock, the wave's lanes striding over it (dwords: GRAY blocks whose rows are dword-aligned)
template <int BPP, typename F>
__device__ __forceinline__ void block_visit(const uint8_t* __restrict__ base, int step, int bs, int blue_shift, int dwords, int lane, F f)
{
    if (BPP == 1 && dwords)
    {
        const int q = bs >> 2, n4 = bs * q;
        for (int i = lane; i < n4; i += 64)
        {
            const int py = i / q, g = i - py * q;
            const uint32_t v = *reinterpret_cast<const uint32_t*>(base + (size_t)py * step + g * 4);
            f(byte_of(v, 0)); f(byte_of(v, 1)); f(byte_of(v, 2)); f(byte_of(v, 3));
        }
        return;
    }
    const int n = bs * bs;
    for (int i = lane; i < n; i += 64)
    {
        const int py = i / bs, px = i - py * bs;
        f(gray_of<BPP>(load_pixel<BPP>(base + (size_t)py * step + px * BPP), blue_shift));
    }
}

// one wave per macroblock (4 per block of 256 threads along x)
template <int BPP>
__global__ __launch_bounds__(256)
void k_deblock_stats(const uint8_t* __restrict__ frame, int step, int blue_shift, int bs, int ex, float inv_area, int levels, double level_step,
                     int dwords, uint8_t* __restrict__ mean_out, uint8_t* __restrict__ grid_out, float* __restrict__ keep_out)
{
    const int lane = threadIdx.x & 63;
    const int bx = blockIdx.x * 4 + (threadIdx.x >> 6), by = blockIdx.y;
    if (bx >= ex) return;                       // whole waves only
    const uint8_t* base = frame + (size_t)by * bs * step + (size_t)bx * bs * BPP;
    block_stats([&](auto f) { block_visit<BPP>(base, step, bs, blue_shift, dwords, lane, f); }, bs, inv_area, levels, level_step, lane,
                (size_t)by * ex + bx, mean_out, grid_out, keep_out);
}

// INTER_AREA of the region (BPP channels) to hs x ws, one thread per output pixel: down_pixel of deblock_core.hpp on the packed frame's pixels
template <int BPP>
__global__ __launch_bounds__(256)
void k_deblock_down(const uint8_t* __restrict__ src, int step, int rh, int rw, uint8_t* __restrict__ dst, int hs, int ws,
                    int iscale, float inv_area, const int2* __restrict__ xr, const AreaTabEntry* __restrict__ xt,
                    const int2* __restrict__ yr, const AreaTabEntry* __restrict__ yt)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= ws || y >= hs) return;
    uint8_t* d = dst + ((size_t)y * ws + x) * BPP;
    down_pixel<BPP>([&](int yy) { return src + (size_t)yy * step; }, [](const uint8_t* r, int xx) { return load_pixel<BPP>(r + (size_t)xx * BPP); },
                    d, x, y, rh, rw, iscale, inv_area, xr, xt, yr, yt);
}

template <int BPP>
__device__ __forceinline__ uint32_t load_clamped(const uint8_t* __restrict__ src, int rows, int cols, int y, int x)      // BORDER_REPLICATE
{
    y = min(max(y, 0), rows - 1); x = min(max(x, 0), cols - 1);
    return load_pixel<BPP>(src + ((size_t)y * cols + x) * BPP);
}

// Rank `mid` of each of NC channels by radix selection: the largest v with #(values < v) <= mid, found bit by bit from the top
// (N > 0: the window size is a compile-time constant and the counting loops unroll over a register window)
template <int NC, int N, typename Get>
__device__ __forceinline__ uint32_t radix_select(int n_rt, Get get)
{
    const int n = N ? N : n_rt, mid = n / 2;
    int p[NC] = {};
    for (int bit = 7; bit >= 0; bit--)
    {
        int cand[NC], cnt[NC] = {};
#pragma unroll
        for (int c = 0; c < NC; c++) cand[c] = p[c] | (1 << bit);
        auto count = [&](int i) {
            const uint32_t v = get(i);
#pragma unroll
            for (int c = 0; c < NC; c++) cnt[c] += byte_of(v, c) < cand[c];
        };
        if constexpr (N > 0)
        {
#pragma unroll
            for (int i = 0; i < N; i++) count(i);
        }
        else
            for (int i = 0; i < n; i++) count(i);
#pragma unroll
        for (int c = 0; c < NC; c++)
            if (cnt[c] <= mid) p[c] = cand[c];
    }
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < NC; c++) out |= (uint32_t)p[c] << (8 * c);
    return out;
}

// the LDS tile: one pixel per element -- a byte for GRAY, a dword for three and four channels
template <int BPP>
__device__ __forceinline__ uint32_t tile_at(const uint32_t* tile, int i)
{
    if constexpr (BPP == 1) return reinterpret_cast<const uint8_t*>(tile)[i];
    else return tile[i];
}

// KS = 3 / 5: the window in registers; KS = 0: run-time k over the LDS tile (use_lds) or straight from global memory (k > kMedLdsMaxK)
template <int BPP, int KS>
__global__ __launch_bounds__(256)
void k_deblock_median(const uint8_t* __restrict__ src, int rows, int cols, uint8_t* __restrict__ dst, int k, int use_lds)
{
    extern __shared__ uint32_t tile[];
    const int kk = KS ? KS : k, r = kk / 2, tw = kMedTile + kk - 1;
    const int x0 = blockIdx.x * kMedTile, y0 = blockIdx.y * kMedTile;
    const int tx = threadIdx.x % kMedTile, ty = threadIdx.x / kMedTile;
    if (use_lds)
    {
        for (int i = threadIdx.x; i < tw * tw; i += 256)
        {
            const int iy = i / tw, ix = i - iy * tw;
            const uint32_t v = load_clamped<BPP>(src, rows, cols, y0 + iy - r, x0 + ix - r);
            if constexpr (BPP == 1) reinterpret_cast<uint8_t*>(tile)[i] = (uint8_t)v;
            else tile[i] = v;
        }
        __syncthreads();
    }
    const int x = x0 + tx, y = y0 + ty;
    if (x >= cols || y >= rows) return;
    const int n = kk * kk;
    uint32_t m;
    if constexpr (KS > 0)
    {
        uint32_t w[KS * KS];
#pragma unroll
        for (int dy = 0; dy < KS; dy++)
#pragma unroll
            for (int dx = 0; dx < KS; dx++) w[dy * KS + dx] = tile_at<BPP>(tile, (ty + dy) * tw + tx + dx);
        m = radix_select<BPP, KS * KS>(n, [&](int i) { return w[i]; });
    }
    else if (use_lds)
        m = radix_select<BPP, 0>(n, [&](int i) { const int dy = i / kk; return tile_at<BPP>(tile, (ty + dy) * tw + tx + i - dy * kk); });
    else
        m = radix_select<BPP, 0>(n, [&](int i) { const int dy = i / kk; return load_clamped<BPP>(src, rows, cols, y + dy - r, x + i - dy * kk - r); });
    store_pixel<BPP>(dst + ((size_t)y * cols + x) * BPP, m);
}

// In place on the region, three and four channels: one thread per pixel.  INFLUENCE: `smooth` is the constant `colour` (draw_influence).
// One loop over the channels, each its `smooth` and then its blend: with all of `smooth` packed first the divisions queue behind every tap, which
// measured 0.4 % slower per four-channel apply at 4K.
template <int BPP, bool INFLUENCE>
__global__ __launch_bounds__(256)
void k_deblock_blend(uint8_t* __restrict__ frame, int step, int rh, int rw,
                     const float* __restrict__ keep_block, int ex, const LinTabEntry* __restrict__ kx, const LinTabEntry* __restrict__ ky,
                     const uint8_t* __restrict__ small, int ws, const Lin8Entry* __restrict__ sx, const Lin8Entry* __restrict__ sy, uint32_t colour)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= rw || y >= rh) return;
    const LinTabEntry tyk = ky[y];
    const float keep = keep_at(keep_block + (size_t)tyk.s0 * ex, keep_block + (size_t)tyk.s1 * ex, kx[x], tyk);
    const float deb = fabsf(keep - 1.0f);
    const float den = (keep + deb) + 1e-5f;
    Lin8Entry txs{}, tys{};
    uint32_t p00 = 0, p01 = 0, p10 = 0, p11 = 0;            // the four taps of `smooth`
    if constexpr (!INFLUENCE)
    {
        txs = sx[x]; tys = sy[y];
        const size_t r0 = (size_t)tys.s0 * ws, r1 = (size_t)tys.s1 * ws;        // the two rows of `small`, in pixels
        p00 = load_pixel<BPP>(small + (r0 + txs.s0) * BPP); p01 = load_pixel<BPP>(small + (r0 + txs.s1) * BPP);
        p10 = load_pixel<BPP>(small + (r1 + txs.s0) * BPP); p11 = load_pixel<BPP>(small + (r1 + txs.s1) * BPP);
    }
    uint8_t* p = frame + (size_t)y * step + (size_t)x * BPP;
    const uint32_t v = load_pixel<BPP>(p);
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < BPP; c++)
    {
        const int s = INFLUENCE ? byte_of(colour, c) : lin8(byte_of(p00, c), byte_of(p01, c), byte_of(p10, c), byte_of(p11, c), txs, tys.a0, tys.a1);
        out |= (uint32_t)blend_px(byte_of(v, c), s, keep, deb, den) << (8 * c);
    }
    store_pixel<BPP>(p, out);
}

// In place on the region, GRAY: one thread per dword-aligned group of four pixels
__global__ __launch_bounds__(256)
void k_deblock_blend_gray(uint8_t* __restrict__ frame, int step, int rh, int rw,
                          const float* __restrict__ keep_block, int ex, const LinTabEntry* __restrict__ kx, const LinTabEntry* __restrict__ ky,
                          const uint8_t* __restrict__ small, int ws, const Lin8Entry* __restrict__ sx, const Lin8Entry* __restrict__ sy)
{
    const int g = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (y >= rh) return;
    uint8_t* row = frame + (size_t)y * step;
    const int x0 = g * 4 - (int)((uintptr_t)row & 3u);       // the group's first pixel: row + x0 is a dword boundary; x0 >= -3
    if (x0 >= rw) return;
    const bool whole = x0 >= 0 && x0 + 4 <= rw;              // else: the row starts or the region ends inside the group
    const LinTabEntry tyk = ky[y];
    const float* k0 = keep_block + (size_t)tyk.s0 * ex;
    const float* k1 = keep_block + (size_t)tyk.s1 * ex;
    const Lin8Entry tys = sy[y];
    const uint8_t* r0 = small + (size_t)tys.s0 * ws;
    const uint8_t* r1 = small + (size_t)tys.s1 * ws;
    uint32_t v = 0;
    if (whole) v = *reinterpret_cast<const uint32_t*>(row + x0);
    else
    {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (x0 + j >= 0 && x0 + j < rw) v |= (uint32_t)row[x0 + j] << (8 * j);
    }
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
    {
        const int x = x0 + j;
        if (!whole && (x < 0 || x >= rw)) continue;
        const float keep = keep_at(k0, k1, kx[x], tyk);
        const float deb = fabsf(keep - 1.0f);
        const float den = (keep + deb) + 1e-5f;
        const Lin8Entry txs = sx[x];
        const int s = lin8(r0[txs.s0], r0[txs.s1], r1[txs.s0], r1[txs.s1], txs, tys.a0, tys.a1);
        out |= (uint32_t)blend_px(byte_of(v, j), s, keep, deb, den) << (8 * j);
    }
    if (whole) *reinterpret_cast<uint32_t*>(row + x0) = out;
    else
    {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (x0 + j >= 0 && x0 + j < rw) row[x0 + j] = (uint8_t)(out >> (8 * j));
    }
}

bool settings_valid(const lvk_deblock_settings& s)
{
    return s.block_size > 0 && s.filter_size >= 3 && s.filter_size % 2 == 1 && s.detection_levels > 0 && s.filter_scaling > 1.0f;
}

// the block statistics of `frame` (BPP bytes per pixel, its grey by `format`) into the handle's grids
template <int BPP>
int launch_stats(lvk_hip_deblock* d, const uint8_t* frame, int step, int format, const Geometry& g)
{
    lvk_hip_ctx* ctx = d->ctx;
    const lvk_deblock_settings& s = d->settings;
    const size_t cells = (size_t)g.ey * g.ex;
    const float inv_area_bs = 1.0f / (float)((long long)g.bs * g.bs);
    const int blue_shift = format == LVK_FORMAT_YUV ? -1 : format == LVK_FORMAT_RGB || format == LVK_FORMAT_RGBA ? 16 : 0;     // gray_of
    const int dwords = BPP == 1 && g.bs % 4 == 0 && ((uintptr_t)frame & 3u) == 0 && (step & 3) == 0;
    hipLaunchKernelGGL(k_deblock_stats<BPP>, dim3((g.ex + 3) / 4, g.ey), dim3(256), 0, ctx->stream, frame, step, blue_shift, g.bs, g.ex,
                       inv_area_bs, (int)std::min<uint32_t>(s.detection_levels, 256u), 1.0 / (double)s.detection_levels, dwords,
                       d->d_grid, d->d_grid + cells, d->d_keep);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

template <int BPP>
int launch_median(lvk_hip_ctx* ctx, const lvk_hip_deblock* d, int hs, int ws, int k)
{
    const dim3 mg((ws + kMedTile - 1) / kMedTile, (hs + kMedTile - 1) / kMedTile);
    const int tw = kMedTile + k - 1;
    const bool lds = k <= kMedLdsMaxK;
    const size_t lds_bytes = !lds ? 0 : BPP == 1 ? ((size_t)tw * tw + 3) / 4 * 4 : (size_t)tw * tw * sizeof(uint32_t);     // tile_at: a byte or a dword per pixel
    if (k == 3)
        hipLaunchKernelGGL((k_deblock_median<BPP, 3>), mg, dim3(256), lds_bytes, ctx->stream, (const uint8_t*)d->d_small, hs, ws, d->d_median, k, 1);
    else if (k == 5)
        hipLaunchKernelGGL((k_deblock_median<BPP, 5>), mg, dim3(256), lds_bytes, ctx->stream, (const uint8_t*)d->d_small, hs, ws, d->d_median, k, 1);
    else
        hipLaunchKernelGGL((k_deblock_median<BPP, 0>), mg, dim3(256), lds_bytes, ctx->stream, (const uint8_t*)d->d_small, hs, ws, d->d_median, k, lds ? 1 : 0);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// the blend of an apply, or (influence, three channels only) draw_influence's: `colour` for `smooth`, no Lin8 tables
template <int BPP>
int launch_blend(lvk_hip_ctx* ctx, uint8_t* frame, int step, const lvk_hip_deblock* d, bool influence = false, uint32_t colour = 0)
{
    const LinTabEntry *kx, *ky;
    const Lin8Entry *sx = nullptr, *sy = nullptr;
    int rc;
    if ((rc = blend_tables(ctx, d, !influence, &kx, &ky, &sx, &sy)) != LVK_HIP_OK) return rc;
    // GRAY: groups of four pixels; a row that starts 1 .. 3 bytes above a dword boundary spreads over one group more
    const int across = BPP == 1 ? (d->rw + 3) / 4 + 1 : d->rw;
    const dim3 grid((across + 63) / 64, (d->rh + 3) / 4), block(64, 4);
    const float* keep = d->d_keep;
    const uint8_t* small = d->d_median;
    if constexpr (BPP == 1)
        hipLaunchKernelGGL(k_deblock_blend_gray, grid, block, 0, ctx->stream, frame, step, d->rh, d->rw, keep, d->ex, kx, ky, small, d->ws, sx, sy);
    else if (BPP == 3 && influence)
        hipLaunchKernelGGL((k_deblock_blend<3, true>), grid, block, 0, ctx->stream, frame, step, d->rh, d->rw, keep, d->ex, kx, ky, small, d->ws, sx, sy, colour);
    else
        hipLaunchKernelGGL((k_deblock_blend<BPP, false>), grid, block, 0, ctx->stream, frame, step, d->rh, d->rw, keep, d->ex, kx, ky, small, d->ws, sx, sy, colour);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// The three entries' apply for BPP bytes per pixel; `who` names the entry in its refusals, `format` is looked at for three and four channels
template <int BPP>
int apply(lvk_hip_deblock* d, void* d_frame, int step, int rows, int cols, int format, int region_xywh[4], const char* who)
{
    if (!d) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = d->ctx;
    LVK_HIP_ENTRY(ctx);
    const lvk_deblock_settings& s = d->settings;
    const std::string name(who);
    if (!(d_frame && rows > 0 && cols > 0 && (long long)step >= (long long)BPP * cols))      // in the words each entry has always reported it
        return ctx->fail(LVK_HIP_ERR_ARG, BPP == 3 ? "pre-condition failed: d_frame && rows > 0 && cols > 0 && (long long)step >= 3LL * cols"
                                                   : "pre-condition failed: d_frame && rows > 0 && cols > 0 && (long long)step >= (long long)BPP * cols");
    if (BPP == 3 && lvk_format_channels(format) != 3) return ctx->fail(LVK_HIP_ERR_ARG, name + ": packed 8UC3 BGR / RGB / YUV frames only");
    if (BPP == 4)
    {
        if (format != LVK_FORMAT_BGRA && format != LVK_FORMAT_RGBA) return ctx->fail(LVK_HIP_ERR_ARG, name + ": packed 8UC4 BGRA / RGBA frames only");
        if (((uintptr_t)d_frame & 3u) || (step & 3))
            return ctx->fail(LVK_HIP_ERR_ARG, name + ": a four-channel frame is 4-byte aligned with a pitch that is a multiple of 4");
    }
    Geometry g;
    int rc;
    if ((rc = geometry(ctx, s, rows, cols, name, g)) != LVK_HIP_OK) return rc;
    if ((rc = reserve(d, g, BPP)) != LVK_HIP_OK) return rc;

    uint8_t* frame = (uint8_t*)d_frame;
    if ((rc = launch_stats<BPP>(d, frame, step, format, g)) != LVK_HIP_OK) return rc;
    const float inv_area_s = g.fast ? 1.0f / (float)((long long)g.iscale * g.iscale) : 0.0f;
    hipLaunchKernelGGL(k_deblock_down<BPP>, dim3((g.ws + 63) / 64, (g.hs + 3) / 4), dim3(64, 4), 0, ctx->stream, (const uint8_t*)frame, step, g.rh, g.rw,
                       d->d_small, g.hs, g.ws, g.fast ? g.iscale : 0, inv_area_s, (const int2*)d->d_xr, (const AreaTabEntry*)d->d_xt,
                       (const int2*)d->d_yr, (const AreaTabEntry*)d->d_yt);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    if ((rc = launch_median<BPP>(ctx, d, g.hs, g.ws, (int)s.filter_size)) != LVK_HIP_OK) return rc;

    d->rh = g.rh; d->rw = g.rw; d->ey = g.ey; d->ex = g.ex; d->hs = g.hs; d->ws = g.ws; d->have_maps = true;
    if ((rc = launch_blend<BPP>(ctx, frame, step, d)) != LVK_HIP_OK) return rc;
    if (region_xywh) { region_xywh[0] = 0; region_xywh[1] = 0; region_xywh[2] = g.rw; region_xywh[3] = g.rh; }
    return LVK_HIP_OK;
}

} // namespace

// deblock_core.hpp: the two launches the 4:2:0 entry (deblock_420.hip) reuses unchanged
int deblock::launch_stats_plane(lvk_hip_deblock* d, const uint8_t* plane, int step, const Geometry& g)
{
    return launch_stats<1>(d, plane, step, LVK_FORMAT_GRAY, g);
}

int deblock::launch_median_c3(lvk_hip_deblock* d, const Geometry& g)
{
    return launch_median<3>(d->ctx, d, g.hs, g.ws, (int)d->settings.filter_size);
}

extern "C" {

void lvk_hip_deblock_default_settings(lvk_deblock_settings* s)
{
    if (!s) return;
    s->detection_levels = 3; s->block_size = 16; s->filter_size = 5; s->filter_scaling = 4.0f;    // DeblockingFilter.hpp:27-33
}

int lvk_hip_deblock_create(lvk_hip_ctx* ctx, const lvk_deblock_settings* settings, lvk_hip_deblock** out)
{
    if (!ctx || !out) return LVK_HIP_ERR_ARG;
    *out = nullptr;
    lvk_deblock_settings s;
    lvk_hip_deblock_default_settings(&s);
    if (settings) s = *settings;
    if (!settings_valid(s)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_create: invalid settings (DeblockingFilter.cpp:37-41)");
    lvk_hip_deblock* d = new lvk_hip_deblock();
    d->ctx = ctx; d->settings = s;
    *out = d;
    return LVK_HIP_OK;
}

int lvk_hip_deblock_configure(lvk_hip_deblock* d, const lvk_deblock_settings* settings)
{
    if (!d || !settings) return LVK_HIP_ERR_ARG;
    if (!settings_valid(*settings)) return d->ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_configure: invalid settings (DeblockingFilter.cpp:37-41)");
    d->settings = *settings;
    return LVK_HIP_OK;
}

void lvk_hip_deblock_destroy(lvk_hip_deblock* d)
{
    if (!d) return;
    lvk_device_guard guard(d->ctx);
    d->release();                   // back to the context's pool, in its stream order
    delete d;
}

int lvk_hip_deblock_apply(lvk_hip_deblock* d, void* d_frame, int step, int rows, int cols, int format, int region_xywh[4])
{
    return apply<3>(d, d_frame, step, rows, cols, format, region_xywh, "lvk_hip_deblock_apply");
}

int lvk_hip_deblock_apply_gray(lvk_hip_deblock* d, void* d_frame, int step, int rows, int cols, int region_xywh[4])
{
    return apply<1>(d, d_frame, step, rows, cols, LVK_FORMAT_GRAY, region_xywh, "lvk_hip_deblock_apply_gray");
}

int lvk_hip_deblock_apply_c4(lvk_hip_deblock* d, void* d_frame, int step, int rows, int cols, int format, int region_xywh[4])
{
    return apply<4>(d, d_frame, step, rows, cols, format, region_xywh, "lvk_hip_deblock_apply_c4");
}

int lvk_hip_deblock_draw_influence(const lvk_hip_deblock* d, void* d_frame, int step, int rows, int cols, int format)
{
    if (!d) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = d->ctx;
    LVK_HIP_ENTRY(ctx);
    if (!d->have_maps) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_draw_influence: no blend maps before the first apply (DeblockingFilter.cpp:116)");
    LVK_HIP_REQUIRE(ctx, d_frame && rows > 0 && cols > 0 && (long long)step >= 3LL * cols);
    if (lvk_format_channels(format) != 3) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_draw_influence: packed 8UC3 BGR / RGB / YUV frames only");
    if (d->rw > cols || d->rh > rows) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_draw_influence: the filter region does not fit the frame (DeblockingFilter.cpp:117-118)");
    // lvk::col::MAGENTA[frame.format] (Functions/Drawing.hpp), byte 0 first: {105, 212, 234} for YUV, else {255, 0, 255}
    const uint32_t magenta = format == LVK_FORMAT_YUV ? 105u | (212u << 8) | (234u << 16) : 255u | (0u << 8) | (255u << 16);
    return launch_blend<3>(ctx, (uint8_t*)d_frame, step, d, true, magenta);
}

int lvk_hip_deblock_filter_region(const lvk_hip_deblock* d, int region_xywh[4])
{
    if (!d || !region_xywh) return LVK_HIP_ERR_ARG;
    region_xywh[0] = 0; region_xywh[1] = 0; region_xywh[2] = d->rw; region_xywh[3] = d->rh;
    return LVK_HIP_OK;
}

int lvk_hip_deblock_get_grid(lvk_hip_deblock* d, uint8_t* mean, uint8_t* grid, float* keep_block, int capacity, int extent_xy[2])
{
    if (!d) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = d->ctx;
    LVK_HIP_ENTRY(ctx);
    if (!d->have_maps) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_get_grid: nothing applied yet");
    const size_t cells = (size_t)d->ey * d->ex;
    if (extent_xy) { extent_xy[0] = d->ex; extent_xy[1] = d->ey; }
    LVK_HIP_REQUIRE(ctx, capacity >= 0 && (size_t)capacity >= cells);
    LVK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (mean) LVK_HIP_CHECK(ctx, hipMemcpy(mean, d->d_grid, cells, hipMemcpyDeviceToHost));
    if (grid) LVK_HIP_CHECK(ctx, hipMemcpy(grid, d->d_grid + cells, cells, hipMemcpyDeviceToHost));
    if (keep_block) LVK_HIP_CHECK(ctx, hipMemcpy(keep_block, d->d_keep, cells * sizeof(float), hipMemcpyDeviceToHost));
    return (int)cells;
}

} // extern "C"
