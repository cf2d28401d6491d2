// lvk::DeblockingFilter on ONE-channel (8UC1, VideoFrame::GRAY) and FOUR-channel (8UC4, VideoFrame::BGRA / RGBA) frames for gfx950: the kernels
// behind lvk_hip_deblock_apply_gray / _c4.  Specification: tests/np_deblock_px.py and DESIGN.md section 23.
//
// The reference's filter is made of channel-agnostic OpenCV calls (Filters/DeblockingFilter.cpp:48-110: cv::resize, cv::medianBlur, reformatTo(GRAY),
// cv::blendLinear), so both pixel sizes are the reference's own: the operation order and every rounding of deblock.hip, per channel.
//   GRAY: the grey image of the block statistics is the frame itself.
//   Four channels: the grey is the fixed-point BT.601 of the three colour bytes (BGRA2GRAY / RGBA2GRAY, alpha ignored).  The ALPHA byte is a channel
//     like the others -- downscaled, median-filtered, up-sampled and blended under the same `keep` map --, because that is what those calls do to an
//     8UC4 UMat.  This differs on purpose from lvk_hip_sharpen_c4 and the four-channel remap, whose alpha had no reference program and was defined here.
//
// The four kernels of deblock.hip with the bytes per pixel (BPP = 1 / 4) as a template parameter, all on the context's stream, nothing synchronises:
//   k_deblock_stats_px   one wave per macroblock.  Four channels: one dword per pixel, the grey from its bytes (the format selects which byte is blue).
//                        GRAY: one dword per four pixels where the block rows are dword-aligned (block size, base and pitch multiples of 4), else bytes.
//   k_deblock_down_px    INTER_AREA of the region, one thread per output pixel and BPP sums: integer box rule (partial cells (float)sum / count) or the
//                        area tables in table order.
//   k_deblock_median_px  the radix selection of deblock.hip with one counter set per channel.  The LDS tile holds one PIXEL per element: a dword (the
//                        four channels packed) for four-channel frames, ONE BYTE for GRAY -- a GRAY tile is a quarter of the size and is read with
//                        byte loads; the register window of k = 3 / 5 holds one pixel per register either way.
//   k_deblock_blend_px   in place on the region.  Four channels: one thread per pixel, one dword load and one dword store, the four taps of `smooth`
//                        as dwords.  GRAY: one thread per group of four pixels; the groups of a row start at the dword boundary at or below the
//                        row's first byte (so every row is aligned whatever the base and the pitch are), a group that lies inside the region is one
//                        dword load and one dword store, the first and the last group of a row go byte by byte over the pixels they hold.
// No load or store touches a byte outside the rw * BPP bytes of a region row, and only the region is written.
#include "deblock_internal.hpp"

using namespace lvk_deblock;

namespace {

__device__ __forceinline__ int sat_u8(float v)           // saturate_cast<uchar>(float): round half to even, clamp
{
    const float r = rintf(v);
    return r < 0.f ? 0 : r > 255.f ? 255 : (int)r;
}

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// resizeAreaFast_ of one block of bs x bs values: 2 x 2 as (sum + 2) >> 2, else sum * (1.f / area) rounded half to even
__device__ __forceinline__ int box_mean(long long sum, int bs, float inv_area)
{
    return bs == 2 ? (int)((sum + 2) >> 2) : sat_u8((float)sum * inv_area);
}

__device__ __forceinline__ int byte_of(uint32_t v, int c) { return (int)((v >> (8 * c)) & 255u); }

// RGB2Gray<uchar> of a four-channel pixel; blue_shift: the bit position of the blue byte (0: BGRA, 16: RGBA), alpha ignored
__device__ __forceinline__ int gray_c4(uint32_t v, int blue_shift)
{
    const int b = (int)((v >> blue_shift) & 255u), g = (int)((v >> 8) & 255u), r = (int)((v >> (16 - blue_shift)) & 255u);
    return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15;
}

template <int BPP>
__device__ __forceinline__ uint32_t load_pixel(const uint8_t* __restrict__ p)       // a pixel's channels in bytes 0 .. BPP - 1
{
    if constexpr (BPP == 4) return *reinterpret_cast<const uint32_t*>(p);
    else return *p;
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
        const uint32_t v = load_pixel<BPP>(base + (size_t)py * step + px * BPP);
        f(BPP == 4 ? gray_c4(v, blue_shift) : (int)v);
    }
}

// one wave per macroblock (4 per block of 256 threads along x)
template <int BPP>
__global__ __launch_bounds__(256)
void k_deblock_stats_px(const uint8_t* __restrict__ frame, int step, int blue_shift, int bs, int ex, float inv_area, int levels, double level_step,
                        int dwords, uint8_t* __restrict__ mean_out, uint8_t* __restrict__ grid_out, float* __restrict__ keep_out)
{
    const int lane = threadIdx.x & 63;
    const int bx = blockIdx.x * 4 + (threadIdx.x >> 6), by = blockIdx.y;
    if (bx >= ex) return;                       // whole waves only
    const uint8_t* base = frame + (size_t)by * bs * step + (size_t)bx * bs * BPP;
    long long sum = 0;
    block_visit<BPP>(base, step, bs, blue_shift, dwords, lane, [&](int g) { sum += g; });
    const int mean = box_mean(wave_sum(sum), bs, inv_area);
    long long dev = 0;                          // the block's bytes are still in L1 / L2: one HBM read for both passes
    block_visit<BPP>(base, step, bs, blue_shift, dwords, lane, [&](int g) { dev += abs(g - mean); });
    const int grid = box_mean(wave_sum(dev), bs, inv_area);
    if (lane == 0)
    {
        const size_t o = (size_t)by * ex + bx;
        mean_out[o] = (uint8_t)mean;
        grid_out[o] = (uint8_t)grid;
        keep_out[o] = (float)((double)min(grid, levels) * level_step);
    }
}

template <int BPP>
__device__ __forceinline__ void store_pixel(uint8_t* __restrict__ p, uint32_t v)
{
    if constexpr (BPP == 4) *reinterpret_cast<uint32_t*>(p) = v;
    else *p = (uint8_t)v;
}

// INTER_AREA of the region (BPP channels) to hs x ws: k_deblock_down of deblock.hip per channel (iscale > 0: integer scale, cells that reach past the
// source average what they cover; iscale == 0: separable area tables, float accumulation in table order)
template <int BPP>
__global__ __launch_bounds__(256)
void k_deblock_down_px(const uint8_t* __restrict__ src, int step, int rh, int rw, uint8_t* __restrict__ dst, int hs, int ws,
                       int iscale, float inv_area, const int2* __restrict__ xr, const AreaTabEntry* __restrict__ xt,
                       const int2* __restrict__ yr, const AreaTabEntry* __restrict__ yt)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= ws || y >= hs) return;
    uint8_t* d = dst + ((size_t)y * ws + x) * BPP;
    uint32_t out = 0;
    if (iscale > 0)
    {
        const int x0 = x * iscale, y0 = y * iscale;
        const int x1 = min(x0 + iscale, rw), y1 = min(y0 + iscale, rh);
        const bool full = x0 + iscale <= rw && y0 + iscale <= rh;
        int s[BPP] = {};
        for (int yy = y0; yy < y1; yy++)
        {
            const uint8_t* r = src + (size_t)yy * step;
            for (int xx = x0; xx < x1; xx++)
            {
                const uint32_t v = load_pixel<BPP>(r + (size_t)xx * BPP);
#pragma unroll
                for (int c = 0; c < BPP; c++) s[c] += byte_of(v, c);
            }
        }
        const float cnt = (float)((x1 - x0) * (y1 - y0));
#pragma unroll
        for (int c = 0; c < BPP; c++)
            out |= (uint32_t)(full ? box_mean(s[c], iscale, inv_area) : sat_u8((float)s[c] / cnt)) << (8 * c);
        store_pixel<BPP>(d, out);
        return;
    }
    const int2 rx = xr[x], ry = yr[y];
    float a[BPP] = {};
    for (int j = 0; j < ry.y; j++)
    {
        const AreaTabEntry ty = yt[ry.x + j];
        const uint8_t* r = src + (size_t)ty.si * step;
        float b[BPP] = {};
        for (int i = 0; i < rx.y; i++)
        {
            const AreaTabEntry tx = xt[rx.x + i];
            const uint32_t v = load_pixel<BPP>(r + (size_t)tx.si * BPP);
#pragma unroll
            for (int c = 0; c < BPP; c++) b[c] = b[c] + (float)byte_of(v, c) * tx.alpha;
        }
#pragma unroll
        for (int c = 0; c < BPP; c++) a[c] = a[c] + ty.alpha * b[c];
    }
#pragma unroll
    for (int c = 0; c < BPP; c++) out |= (uint32_t)sat_u8(a[c]) << (8 * c);
    store_pixel<BPP>(d, out);
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

// the LDS tile: one pixel per element -- a dword for four channels, a byte for GRAY
template <int BPP>
__device__ __forceinline__ uint32_t tile_at(const uint32_t* tile, int i)
{
    if constexpr (BPP == 4) return tile[i];
    else return reinterpret_cast<const uint8_t*>(tile)[i];
}

// KS = 3 / 5: the window in registers; KS = 0: run-time k over the LDS tile (use_lds) or straight from global memory (k > kMedLdsMaxK)
template <int BPP, int KS>
__global__ __launch_bounds__(256)
void k_deblock_median_px(const uint8_t* __restrict__ src, int rows, int cols, uint8_t* __restrict__ dst, int k, int use_lds)
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
            if constexpr (BPP == 4) tile[i] = v;
            else reinterpret_cast<uint8_t*>(tile)[i] = (uint8_t)v;
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

// `keep` of one pixel: the float bilinear of keep_block (k0 / k1: its two rows)
__device__ __forceinline__ float keep_at(const float* __restrict__ k0, const float* __restrict__ k1, const LinTabEntry& tx, const LinTabEntry& ty)
{
    const float h0 = k0[tx.s0] * tx.a0 + k0[tx.s1] * tx.a1;
    const float h1 = k1[tx.s0] * tx.a0 + k1[tx.s1] * tx.a1;
    return h0 * ty.a0 + h1 * ty.a1;
}

// the 8U bilinear of one channel from its four taps (11-bit coefficients, cv::resize INTER_LINEAR on 8U)
__device__ __forceinline__ int lin8(int p00, int p01, int p10, int p11, const Lin8Entry& tx, int b0, int b1)
{
    const int h0 = p00 * tx.a0 + p01 * tx.a1;
    const int h1 = p10 * tx.a0 + p11 * tx.a1;
    return ((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2) & 0xff;
}

// saturate_cast<uchar>((src * keep + smooth * deblock) / (keep + deblock + 1e-5f)); every product / sum is its own rounding (-ffp-contract=off)
__device__ __forceinline__ int blend_px(int c, int s, float keep, float deb, float den)
{
    return sat_u8(((float)c * keep + (float)s * deb) / den);
}

// In place on the region, four channels: one thread per pixel
__global__ __launch_bounds__(256)
void k_deblock_blend_c4(uint8_t* __restrict__ frame, int step, int rh, int rw,
                        const float* __restrict__ keep_block, int ex, const LinTabEntry* __restrict__ kx, const LinTabEntry* __restrict__ ky,
                        const uint8_t* __restrict__ small, int ws, const Lin8Entry* __restrict__ sx, const Lin8Entry* __restrict__ sy)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= rw || y >= rh) return;
    const LinTabEntry tyk = ky[y];
    const float keep = keep_at(keep_block + (size_t)tyk.s0 * ex, keep_block + (size_t)tyk.s1 * ex, kx[x], tyk);
    const float deb = fabsf(keep - 1.0f);
    const float den = (keep + deb) + 1e-5f;
    const Lin8Entry txs = sx[x], tys = sy[y];
    const uint32_t* r0 = reinterpret_cast<const uint32_t*>(small) + (size_t)tys.s0 * ws;
    const uint32_t* r1 = reinterpret_cast<const uint32_t*>(small) + (size_t)tys.s1 * ws;
    const uint32_t p00 = r0[txs.s0], p01 = r0[txs.s1], p10 = r1[txs.s0], p11 = r1[txs.s1];
    uint32_t* p = reinterpret_cast<uint32_t*>(frame + (size_t)y * step) + x;
    const uint32_t v = *p;
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 4; c++)
    {
        const int s = lin8(byte_of(p00, c), byte_of(p01, c), byte_of(p10, c), byte_of(p11, c), txs, tys.a0, tys.a1);
        out |= (uint32_t)blend_px(byte_of(v, c), s, keep, deb, den) << (8 * c);
    }
    *p = out;
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

template <int BPP>
int launch_median(lvk_hip_ctx* ctx, const lvk_hip_deblock* d, int hs, int ws, int k)
{
    const dim3 mg((ws + kMedTile - 1) / kMedTile, (hs + kMedTile - 1) / kMedTile);
    const int tw = kMedTile + k - 1;
    const bool lds = k <= kMedLdsMaxK;
    const size_t lds_bytes = lds ? ((size_t)tw * tw * BPP + 3) / 4 * 4 : 0;
    if (k == 3)
        hipLaunchKernelGGL((k_deblock_median_px<BPP, 3>), mg, dim3(256), lds_bytes, ctx->stream, (const uint8_t*)d->d_small, hs, ws, d->d_median, k, 1);
    else if (k == 5)
        hipLaunchKernelGGL((k_deblock_median_px<BPP, 5>), mg, dim3(256), lds_bytes, ctx->stream, (const uint8_t*)d->d_small, hs, ws, d->d_median, k, 1);
    else
        hipLaunchKernelGGL((k_deblock_median_px<BPP, 0>), mg, dim3(256), lds_bytes, ctx->stream, (const uint8_t*)d->d_small, hs, ws, d->d_median, k, lds ? 1 : 0);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

template <int BPP>
int launch_blend(lvk_hip_ctx* ctx, uint8_t* frame, int step, const lvk_hip_deblock* d)
{
    const LinTabEntry *kx, *ky;
    const Lin8Entry *sx, *sy;
    int rc;
    if ((rc = lvk_get_lintab(ctx, d->ex, d->rw, false, &kx)) != LVK_HIP_OK) return rc;
    if ((rc = lvk_get_lintab(ctx, d->ey, d->rh, true, &ky)) != LVK_HIP_OK) return rc;
    if ((rc = lvk_get_lin8tab(ctx, d->ws, d->rw, false, &sx)) != LVK_HIP_OK) return rc;
    if ((rc = lvk_get_lin8tab(ctx, d->hs, d->rh, true, &sy)) != LVK_HIP_OK) return rc;
    const dim3 block(64, 4);
    if (BPP == 4)
        hipLaunchKernelGGL(k_deblock_blend_c4, dim3((d->rw + 63) / 64, (d->rh + 3) / 4), block, 0, ctx->stream, frame, step, d->rh, d->rw,
                           (const float*)d->d_keep, d->ex, kx, ky, (const uint8_t*)d->d_median, d->ws, sx, sy);
    else
    {
        const int groups = (d->rw + 3) / 4 + 1;      // a row that starts 1 .. 3 bytes above a dword boundary spreads over one group more
        hipLaunchKernelGGL(k_deblock_blend_gray, dim3((groups + 63) / 64, (d->rh + 3) / 4), block, 0, ctx->stream, frame, step, d->rh, d->rw,
                           (const float*)d->d_keep, d->ex, kx, ky, (const uint8_t*)d->d_median, d->ws, sx, sy);
    }
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// lvk_hip_deblock_apply of deblock.hip for BPP bytes per pixel; `format` is looked at for four channels only
template <int BPP>
int apply_px(lvk_hip_deblock* d, void* d_frame, int step, int rows, int cols, int format, int region_xywh[4], const char* who)
{
    if (!d) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = d->ctx;
    LVK_HIP_ENTRY(ctx);
    const lvk_deblock_settings& s = d->settings;
    const std::string name(who);
    LVK_HIP_REQUIRE(ctx, d_frame && rows > 0 && cols > 0 && (long long)step >= (long long)BPP * cols);
    if (BPP == 4)
    {
        if (format != LVK_FORMAT_BGRA && format != LVK_FORMAT_RGBA) return ctx->fail(LVK_HIP_ERR_ARG, name + ": packed 8UC4 BGRA / RGBA frames only");
        if (((uintptr_t)d_frame & 3u) || (step & 3))
            return ctx->fail(LVK_HIP_ERR_ARG, name + ": a four-channel frame is 4-byte aligned with a pitch that is a multiple of 4");
    }
    LVK_HIP_REQUIRE(ctx, s.filter_size <= (uint32_t)kMaxFilterSize);
    const int bs = s.block_size > (uint32_t)std::max(rows, cols) ? 0 : (int)s.block_size;
    const int ex = bs ? cols / bs : 0, ey = bs ? rows / bs : 0;
    if (ex == 0 || ey == 0) return ctx->fail(LVK_HIP_ERR_ARG, name + ": the frame holds no whole macroblock (cv::resize of an empty region)");
    const int rw = ex * bs, rh = ey * bs;
    const int ws = small_extent(rw, s.filter_scaling), hs = small_extent(rh, s.filter_scaling);
    if (ws == 0 || hs == 0) return ctx->fail(LVK_HIP_ERR_ARG, name + ": the 1 / filter_scaling downscale of the region is empty");

    // downscale mode: resizeAreaFast_ when 1 / (double)(1.f / s) is an integer, else the area tables of that scale
    const double scale = 1.0 / (double)(1.0f / s.filter_scaling);
    const int iscale = (int)std::lrint(scale);
    const bool fast = std::fabs(scale - iscale) < 2.220446049250313e-16;

    int rc;
    const size_t sb = (size_t)hs * ws * BPP, cells = (size_t)ey * ex;
    if ((rc = ensure(ctx, (void**)&d->d_small, d->small_cap, sb)) != LVK_HIP_OK) return rc;
    if ((rc = ensure(ctx, (void**)&d->d_median, d->median_cap, sb)) != LVK_HIP_OK) return rc;
    if ((rc = ensure(ctx, (void**)&d->d_grid, d->grid_cap, cells * 2)) != LVK_HIP_OK) return rc;
    if ((rc = ensure(ctx, (void**)&d->d_keep, d->keep_cap, cells * sizeof(float))) != LVK_HIP_OK) return rc;
    if (!fast && (rc = upload_area_tabs(d, rh, rw, hs, ws, scale)) != LVK_HIP_OK) return rc;

    uint8_t* frame = (uint8_t*)d_frame;
    const float inv_area_bs = 1.0f / (float)((long long)bs * bs);
    const int dwords = BPP == 1 && bs % 4 == 0 && ((uintptr_t)d_frame & 3u) == 0 && (step & 3) == 0;
    hipLaunchKernelGGL(k_deblock_stats_px<BPP>, dim3((ex + 3) / 4, ey), dim3(256), 0, ctx->stream, (const uint8_t*)frame, step,
                       format == LVK_FORMAT_RGBA ? 16 : 0, bs, ex, inv_area_bs, (int)std::min<uint32_t>(s.detection_levels, 256u),
                       1.0 / (double)s.detection_levels, dwords, d->d_grid, d->d_grid + cells, d->d_keep);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    const float inv_area_s = fast ? 1.0f / (float)((long long)iscale * iscale) : 0.0f;
    hipLaunchKernelGGL(k_deblock_down_px<BPP>, dim3((ws + 63) / 64, (hs + 3) / 4), dim3(64, 4), 0, ctx->stream, (const uint8_t*)frame, step, rh, rw,
                       d->d_small, hs, ws, fast ? iscale : 0, inv_area_s, (const int2*)d->d_xr, (const AreaTabEntry*)d->d_xt,
                       (const int2*)d->d_yr, (const AreaTabEntry*)d->d_yt);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    if ((rc = launch_median<BPP>(ctx, d, hs, ws, (int)s.filter_size)) != LVK_HIP_OK) return rc;

    d->rh = rh; d->rw = rw; d->ey = ey; d->ex = ex; d->hs = hs; d->ws = ws; d->have_maps = true;
    if ((rc = launch_blend<BPP>(ctx, frame, step, d)) != LVK_HIP_OK) return rc;
    if (region_xywh) { region_xywh[0] = 0; region_xywh[1] = 0; region_xywh[2] = rw; region_xywh[3] = rh; }
    return LVK_HIP_OK;
}

} // namespace

extern "C" {

int lvk_hip_deblock_apply_gray(lvk_hip_deblock* d, void* d_frame, int step, int rows, int cols, int region_xywh[4])
{
    return apply_px<1>(d, d_frame, step, rows, cols, LVK_FORMAT_GRAY, region_xywh, "lvk_hip_deblock_apply_gray");
}

int lvk_hip_deblock_apply_c4(lvk_hip_deblock* d, void* d_frame, int step, int rows, int cols, int format, int region_xywh[4])
{
    return apply_px<4>(d, d_frame, step, rows, cols, format, region_xywh, "lvk_hip_deblock_apply_c4");
}

} // extern "C"
