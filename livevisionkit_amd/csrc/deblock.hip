// lvk::DeblockingFilter (Filters/DeblockingFilter.{hpp,cpp}) on the MI355X: the adaptive blend of a median-smoothed frame into the
// original, in place on a packed 8UC3 frame.  Specification: tests/np_deblock.py and DESIGN.md section 13.
//
// Four kernels per apply, all on the context's stream, nothing synchronises:
//   k_deblock_stats    one wave per macroblock: exact integer block mean, mean absolute deviation from it (second pass over the same,
//                      cache-resident bytes), keep_block = float(min(grid, L) * (1.0 / L)).
//   k_deblock_down     INTER_AREA of the region by 1 / filter_scaling, 3 channels: integer box rule at integer scales, area tables else.
//   k_deblock_median   exact per-channel median of the k x k window (BORDER_REPLICATE) on the small frame: LDS tile with a replicated
//                      apron, a radix selection (8 counting passes) over a register window for k = 3 / 5, over the tile for larger k.
//   k_deblock_blend    rebuilds `smooth` (8U bilinear from the median frame) and `keep` (float bilinear from keep_block) per pixel and
//                      writes the blend in place; the full-size smooth / keep / deblock frames of the reference are never materialised.
// draw_influence is k_deblock_blend with a constant colour for `smooth` and the keep_block of the last apply.
#include "deblock_internal.hpp"

using namespace lvk_deblock;        // the handle's host side, shared with deblock_px.hip

namespace {

__device__ __forceinline__ int gray_of(const uint8_t* p, int fmt)
{
    if (fmt == LVK_FORMAT_YUV) return p[0];
    const int b = fmt == LVK_FORMAT_BGR ? p[0] : p[2], g = p[1], r = fmt == LVK_FORMAT_BGR ? p[2] : p[0];
    return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15;
}

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

// one wave per macroblock (4 per block of 256 threads along x)
__global__ __launch_bounds__(256)
void k_deblock_stats(const uint8_t* __restrict__ frame, int step, int fmt, int bs, int ex, float inv_area, int levels, double level_step,
                     uint8_t* __restrict__ mean_out, uint8_t* __restrict__ grid_out, float* __restrict__ keep_out)
{
    const int lane = threadIdx.x & 63;
    const int bx = blockIdx.x * 4 + (threadIdx.x >> 6), by = blockIdx.y;
    if (bx >= ex) return;                       // whole waves only
    const uint8_t* base = frame + (size_t)by * bs * step + (size_t)bx * bs * 3;
    const int n = bs * bs;
    long long sum = 0;
    for (int i = lane; i < n; i += 64)
    {
        const int py = i / bs, px = i - py * bs;
        sum += gray_of(base + (size_t)py * step + px * 3, fmt);
    }
    const int mean = box_mean(wave_sum(sum), bs, inv_area);
    long long dev = 0;
    for (int i = lane; i < n; i += 64)          // the block's bytes are still in L1 / L2: one HBM read for both passes
    {
        const int py = i / bs, px = i - py * bs;
        dev += abs(gray_of(base + (size_t)py * step + px * 3, fmt) - mean);
    }
    const int grid = box_mean(wave_sum(dev), bs, inv_area);
    if (lane == 0)
    {
        const size_t o = (size_t)by * ex + bx;
        mean_out[o] = (uint8_t)mean;
        grid_out[o] = (uint8_t)grid;
        keep_out[o] = (float)((double)min(grid, levels) * level_step);
    }
}

// INTER_AREA of the region (3 channels) to hs x ws.  iscale > 0: integer scale (resizeAreaFast_; cells that reach past the source -- a
// destination size rounded up -- average what they cover, (float)sum / count); iscale == 0: separable area tables, float accumulation in
// table order (per source row the x taps, then the rows weighted by their beta).
__global__ __launch_bounds__(256)
void k_deblock_down(const uint8_t* __restrict__ src, int step, int rh, int rw, uint8_t* __restrict__ dst, int hs, int ws,
                    int iscale, float inv_area, const int2* __restrict__ xr, const AreaTabEntry* __restrict__ xt,
                    const int2* __restrict__ yr, const AreaTabEntry* __restrict__ yt)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= ws || y >= hs) return;
    uint8_t* d = dst + ((size_t)y * ws + x) * 3;
    if (iscale > 0)
    {
        const int x0 = x * iscale, y0 = y * iscale;
        const int x1 = min(x0 + iscale, rw), y1 = min(y0 + iscale, rh);
        const bool full = x0 + iscale <= rw && y0 + iscale <= rh;
        int s0 = 0, s1 = 0, s2 = 0;
        for (int yy = y0; yy < y1; yy++)
        {
            const uint8_t* r = src + (size_t)yy * step;
            for (int xx = x0; xx < x1; xx++) { s0 += r[xx * 3]; s1 += r[xx * 3 + 1]; s2 += r[xx * 3 + 2]; }
        }
        if (full)
        {
            d[0] = (uint8_t)box_mean(s0, iscale, inv_area); d[1] = (uint8_t)box_mean(s1, iscale, inv_area); d[2] = (uint8_t)box_mean(s2, iscale, inv_area);
        }
        else
        {
            const float cnt = (float)((x1 - x0) * (y1 - y0));
            d[0] = (uint8_t)sat_u8((float)s0 / cnt); d[1] = (uint8_t)sat_u8((float)s1 / cnt); d[2] = (uint8_t)sat_u8((float)s2 / cnt);
        }
        return;
    }
    const int2 rx = xr[x], ry = yr[y];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int j = 0; j < ry.y; j++)
    {
        const AreaTabEntry ty = yt[ry.x + j];
        const uint8_t* r = src + (size_t)ty.si * step;
        float b0 = 0.f, b1 = 0.f, b2 = 0.f;
        for (int i = 0; i < rx.y; i++)
        {
            const AreaTabEntry tx = xt[rx.x + i];
            const uint8_t* p = r + tx.si * 3;
            b0 = b0 + (float)p[0] * tx.alpha; b1 = b1 + (float)p[1] * tx.alpha; b2 = b2 + (float)p[2] * tx.alpha;
        }
        a0 = a0 + ty.alpha * b0; a1 = a1 + ty.alpha * b1; a2 = a2 + ty.alpha * b2;
    }
    d[0] = (uint8_t)sat_u8(a0); d[1] = (uint8_t)sat_u8(a1); d[2] = (uint8_t)sat_u8(a2);
}

__device__ __forceinline__ uint32_t load_px(const uint8_t* __restrict__ src, int rows, int cols, int y, int x)
{
    y = min(max(y, 0), rows - 1); x = min(max(x, 0), cols - 1);
    const uint8_t* p = src + ((size_t)y * cols + x) * 3;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// Rank `mid` of every channel by radix selection: the largest v with #(values < v) <= mid, found bit by bit from the top
// (N > 0: the window size is a compile-time constant and the counting loops unroll over a register window)
template <int N, typename Get>
__device__ __forceinline__ uint32_t radix_select3(int n_rt, Get get)
{
    const int n = N ? N : n_rt, mid = n / 2;
    int p0 = 0, p1 = 0, p2 = 0;
    for (int bit = 7; bit >= 0; bit--)
    {
        const int c0 = p0 | (1 << bit), c1 = p1 | (1 << bit), c2 = p2 | (1 << bit);
        int n0 = 0, n1 = 0, n2 = 0;
        auto count = [&](int i) {
            const uint32_t v = get(i);
            n0 += (int)(v & 255u) < c0; n1 += (int)((v >> 8) & 255u) < c1; n2 += (int)((v >> 16) & 255u) < c2;
        };
        if constexpr (N > 0)
        {
#pragma unroll
            for (int i = 0; i < N; i++) count(i);
        }
        else
            for (int i = 0; i < n; i++) count(i);
        if (n0 <= mid) p0 = c0;
        if (n1 <= mid) p1 = c1;
        if (n2 <= mid) p2 = c2;
    }
    return (uint32_t)p0 | ((uint32_t)p1 << 8) | ((uint32_t)p2 << 16);
}

// KS = 3 / 5: the window in registers; KS = 0: run-time k over the LDS tile (use_lds) or straight from global memory (k > kMedLdsMaxK)
template <int KS>
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
            tile[i] = load_px(src, rows, cols, y0 + iy - r, x0 + ix - r);
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
            for (int dx = 0; dx < KS; dx++) w[dy * KS + dx] = tile[(ty + dy) * tw + tx + dx];
        m = radix_select3<KS * KS>(n, [&](int i) { return w[i]; });
    }
    else if (use_lds)
        m = radix_select3<0>(n, [&](int i) { const int dy = i / kk; return tile[(ty + dy) * tw + tx + i - dy * kk]; });
    else
        m = radix_select3<0>(n, [&](int i) { const int dy = i / kk; return load_px(src, rows, cols, y + dy - r, x + i - dy * kk - r); });
    uint8_t* d = dst + ((size_t)y * cols + x) * 3;
    d[0] = (uint8_t)(m & 255u); d[1] = (uint8_t)((m >> 8) & 255u); d[2] = (uint8_t)((m >> 16) & 255u);
}

__device__ __forceinline__ int lin8(const uint8_t* __restrict__ r0, const uint8_t* __restrict__ r1, int c, const Lin8Entry& tx, int b0, int b1)
{
    const int h0 = r0[tx.s0 * 3 + c] * tx.a0 + r0[tx.s1 * 3 + c] * tx.a1;
    const int h1 = r1[tx.s0 * 3 + c] * tx.a0 + r1[tx.s1 * 3 + c] * tx.a1;
    return ((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2) & 0xff;
}

// In place on the region: dst = saturate_cast<uchar>((src * keep + smooth * deblock) / (keep + deblock + 1e-5f)).
// INFLUENCE: smooth = the constant colour (draw_influence).  Every product / sum is its own rounding (-ffp-contract=off).
template <bool INFLUENCE>
__global__ __launch_bounds__(256)
void k_deblock_blend(uint8_t* __restrict__ frame, int step, int rh, int rw,
                     const float* __restrict__ keep_block, int ex, const LinTabEntry* __restrict__ kx, const LinTabEntry* __restrict__ ky,
                     const uint8_t* __restrict__ small, int ws, const Lin8Entry* __restrict__ sx, const Lin8Entry* __restrict__ sy,
                     uint8_t m0, uint8_t m1, uint8_t m2)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= rw || y >= rh) return;
    const LinTabEntry tx = kx[x], tyk = ky[y];
    const float* k0 = keep_block + (size_t)tyk.s0 * ex;
    const float* k1 = keep_block + (size_t)tyk.s1 * ex;
    const float h0 = k0[tx.s0] * tx.a0 + k0[tx.s1] * tx.a1;
    const float h1 = k1[tx.s0] * tx.a0 + k1[tx.s1] * tx.a1;
    const float keep = h0 * tyk.a0 + h1 * tyk.a1;
    const float deb = fabsf(keep - 1.0f);
    const float den = (keep + deb) + 1e-5f;
    int s0 = m0, s1 = m1, s2 = m2;
    if (!INFLUENCE)
    {
        const Lin8Entry txs = sx[x], tys = sy[y];
        const uint8_t* r0 = small + (size_t)tys.s0 * ws * 3;
        const uint8_t* r1 = small + (size_t)tys.s1 * ws * 3;
        s0 = lin8(r0, r1, 0, txs, tys.a0, tys.a1); s1 = lin8(r0, r1, 1, txs, tys.a0, tys.a1); s2 = lin8(r0, r1, 2, txs, tys.a0, tys.a1);
    }
    uint8_t* p = frame + (size_t)y * step + (size_t)x * 3;
    const int c0 = p[0], c1 = p[1], c2 = p[2];
    p[0] = (uint8_t)sat_u8(((float)c0 * keep + (float)s0 * deb) / den);
    p[1] = (uint8_t)sat_u8(((float)c1 * keep + (float)s1 * deb) / den);
    p[2] = (uint8_t)sat_u8(((float)c2 * keep + (float)s2 * deb) / den);
}

bool settings_valid(const lvk_deblock_settings& s)
{
    return s.block_size > 0 && s.filter_size >= 3 && s.filter_size % 2 == 1 && s.detection_levels > 0 && s.filter_scaling > 1.0f;
}

bool format_ok(int format) { return format == LVK_FORMAT_BGR || format == LVK_FORMAT_RGB || format == LVK_FORMAT_YUV; }

int launch_blend(lvk_hip_ctx* ctx, bool influence, uint8_t* frame, int step, const lvk_hip_deblock* d, const uint8_t colour[3])
{
    const LinTabEntry *kx, *ky;
    int rc;
    if ((rc = lvk_get_lintab(ctx, d->ex, d->rw, false, &kx)) != LVK_HIP_OK) return rc;
    if ((rc = lvk_get_lintab(ctx, d->ey, d->rh, true, &ky)) != LVK_HIP_OK) return rc;
    const dim3 grid((d->rw + 63) / 64, (d->rh + 3) / 4), block(64, 4);
    if (influence)
        hipLaunchKernelGGL(k_deblock_blend<true>, grid, block, 0, ctx->stream, frame, step, d->rh, d->rw, d->d_keep, d->ex, kx, ky,
                           (const uint8_t*)nullptr, 0, (const Lin8Entry*)nullptr, (const Lin8Entry*)nullptr, colour[0], colour[1], colour[2]);
    else
    {
        const Lin8Entry *sx, *sy;
        if ((rc = lvk_get_lin8tab(ctx, d->ws, d->rw, false, &sx)) != LVK_HIP_OK) return rc;
        if ((rc = lvk_get_lin8tab(ctx, d->hs, d->rh, true, &sy)) != LVK_HIP_OK) return rc;
        hipLaunchKernelGGL(k_deblock_blend<false>, grid, block, 0, ctx->stream, frame, step, d->rh, d->rw, d->d_keep, d->ex, kx, ky,
                           (const uint8_t*)d->d_median, d->ws, sx, sy, (uint8_t)0, (uint8_t)0, (uint8_t)0);
    }
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

} // namespace

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
    if (!d) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = d->ctx;
    LVK_HIP_ENTRY(ctx);
    const lvk_deblock_settings& s = d->settings;
    LVK_HIP_REQUIRE(ctx, d_frame && rows > 0 && cols > 0 && (long long)step >= 3LL * cols);
    if (!format_ok(format)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_apply: packed 8UC3 BGR / RGB / YUV frames only");
    LVK_HIP_REQUIRE(ctx, s.filter_size <= (uint32_t)kMaxFilterSize);
    const int bs = s.block_size > (uint32_t)std::max(rows, cols) ? 0 : (int)s.block_size;
    const int ex = bs ? cols / bs : 0, ey = bs ? rows / bs : 0;
    if (ex == 0 || ey == 0) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_apply: the frame holds no whole macroblock (cv::resize of an empty region)");
    const int rw = ex * bs, rh = ey * bs;
    const int ws = small_extent(rw, s.filter_scaling), hs = small_extent(rh, s.filter_scaling);
    if (ws == 0 || hs == 0) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_apply: the 1 / filter_scaling downscale of the region is empty");

    // downscale mode: resizeAreaFast_ when 1 / (double)(1.f / s) is an integer, else the area tables of that scale
    const double scale = 1.0 / (double)(1.0f / s.filter_scaling);
    const int iscale = (int)std::lrint(scale);
    const bool fast = std::fabs(scale - iscale) < 2.220446049250313e-16;

    int rc;
    const size_t sb = (size_t)hs * ws * 3, cells = (size_t)ey * ex;
    if ((rc = ensure(ctx, (void**)&d->d_small, d->small_cap, sb)) != LVK_HIP_OK) return rc;
    if ((rc = ensure(ctx, (void**)&d->d_median, d->median_cap, sb)) != LVK_HIP_OK) return rc;
    if ((rc = ensure(ctx, (void**)&d->d_grid, d->grid_cap, cells * 2)) != LVK_HIP_OK) return rc;
    if ((rc = ensure(ctx, (void**)&d->d_keep, d->keep_cap, cells * sizeof(float))) != LVK_HIP_OK) return rc;
    if (!fast && (rc = upload_area_tabs(d, rh, rw, hs, ws, scale)) != LVK_HIP_OK) return rc;

    uint8_t* frame = (uint8_t*)d_frame;
    const float inv_area_bs = 1.0f / (float)((long long)bs * bs);
    hipLaunchKernelGGL(k_deblock_stats, dim3((ex + 3) / 4, ey), dim3(256), 0, ctx->stream, (const uint8_t*)frame, step, format, bs, ex,
                       inv_area_bs, (int)std::min<uint32_t>(s.detection_levels, 256u), 1.0 / (double)s.detection_levels,
                       d->d_grid, d->d_grid + cells, d->d_keep);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    const float inv_area_s = fast ? 1.0f / (float)((long long)iscale * iscale) : 0.0f;
    hipLaunchKernelGGL(k_deblock_down, dim3((ws + 63) / 64, (hs + 3) / 4), dim3(64, 4), 0, ctx->stream, (const uint8_t*)frame, step, rh, rw,
                       d->d_small, hs, ws, fast ? iscale : 0, inv_area_s, (const int2*)d->d_xr, (const AreaTabEntry*)d->d_xt,
                       (const int2*)d->d_yr, (const AreaTabEntry*)d->d_yt);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    const int k = (int)s.filter_size;
    const dim3 mg((ws + kMedTile - 1) / kMedTile, (hs + kMedTile - 1) / kMedTile);
    const int tw = kMedTile + k - 1;
    const bool lds = k <= kMedLdsMaxK;
    const size_t lds_bytes = lds ? (size_t)tw * tw * sizeof(uint32_t) : 0;
    if (k == 3)
        hipLaunchKernelGGL(k_deblock_median<3>, mg, dim3(256), lds_bytes, ctx->stream, (const uint8_t*)d->d_small, hs, ws, d->d_median, k, 1);
    else if (k == 5)
        hipLaunchKernelGGL(k_deblock_median<5>, mg, dim3(256), lds_bytes, ctx->stream, (const uint8_t*)d->d_small, hs, ws, d->d_median, k, 1);
    else
        hipLaunchKernelGGL(k_deblock_median<0>, mg, dim3(256), lds_bytes, ctx->stream, (const uint8_t*)d->d_small, hs, ws, d->d_median, k, lds ? 1 : 0);
    LVK_HIP_CHECK(ctx, hipGetLastError());

    d->rh = rh; d->rw = rw; d->ey = ey; d->ex = ex; d->hs = hs; d->ws = ws; d->have_maps = true;
    if ((rc = launch_blend(ctx, false, frame, step, d, nullptr)) != LVK_HIP_OK) return rc;
    if (region_xywh) { region_xywh[0] = 0; region_xywh[1] = 0; region_xywh[2] = rw; region_xywh[3] = rh; }
    return LVK_HIP_OK;
}

int lvk_hip_deblock_draw_influence(const lvk_hip_deblock* d, void* d_frame, int step, int rows, int cols, int format)
{
    if (!d) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = d->ctx;
    LVK_HIP_ENTRY(ctx);
    if (!d->have_maps) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_draw_influence: no blend maps before the first apply (DeblockingFilter.cpp:116)");
    LVK_HIP_REQUIRE(ctx, d_frame && rows > 0 && cols > 0 && (long long)step >= 3LL * cols);
    if (!format_ok(format)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_draw_influence: packed 8UC3 BGR / RGB / YUV frames only");
    if (d->rw > cols || d->rh > rows) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_deblock_draw_influence: the filter region does not fit the frame (DeblockingFilter.cpp:117-118)");
    // lvk::col::MAGENTA[frame.format] (Functions/Drawing.hpp)
    const uint8_t magenta_yuv[3] = {105, 212, 234}, magenta_rgb[3] = {255, 0, 255};
    return launch_blend(ctx, true, (uint8_t*)d_frame, step, d, format == LVK_FORMAT_YUV ? magenta_yuv : magenta_rgb);
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
