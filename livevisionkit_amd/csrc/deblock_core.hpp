// What the deblocking filter's three units share: deblock.hip (packed frames of one, three and four bytes per pixel), deblock_420.hip (I420 / NV12
// planes in and out) and deblock_obs.hip (the planes of the other OBS video formats, section 31).  The handle, the per-pixel
// arithmetic of the specification (tests/np_deblock.py), the two passes of the block statistics with the walk over a block's
// pixels as a parameter, the body of the 1 / filter_scaling downscale with the pixel fetch as a parameter, the geometry of one apply with its
// refusals, the buffers and the area tables.  Every product and sum is its own rounding (-ffp-contract=off).
#pragma once

#include "lvk_hip_internal.hpp"
#include "yuv420_core.hpp"

#include <cmath>
#include <algorithm>
#include <string>
#include <vector>

int lvk_get_lin8tab(lvk_hip_ctx* ctx, int ssize, int dsize, bool vertical, const Lin8Entry** d_out);   // ingest.hip

struct lvk_hip_deblock
{
    lvk_hip_ctx* ctx = nullptr;
    lvk_deblock_settings settings{};
    // geometry of the last apply (draw_influence reuses its maps)
    int rh = 0, rw = 0, ey = 0, ex = 0, hs = 0, ws = 0;
    bool have_maps = false;
    // device buffers, sized in bytes for the geometry and pixel size they were last allocated for (lvk_hip_malloc pool of the context)
    uint8_t* d_small = nullptr; uint8_t* d_median = nullptr; size_t small_cap = 0, median_cap = 0;
    uint8_t* d_grid = nullptr; float* d_keep = nullptr; size_t grid_cap = 0, keep_cap = 0;       // d_grid: mean (cells) | grid (cells)
    // area tables of the non-integer downscale, keyed by (rh, rw, hs, ws, scale)
    int2* d_range = nullptr; AreaTabEntry* d_tab = nullptr; size_t range_cap = 0, tab_cap = 0;
    int2* d_xr = nullptr; int2* d_yr = nullptr; AreaTabEntry* d_xt = nullptr; AreaTabEntry* d_yt = nullptr;
    int tab_rh = -1, tab_rw = -1, tab_hs = -1, tab_ws = -1; double tab_scale = 0.0;

    void release()
    {
        lvk_hip_free(ctx, d_small); lvk_hip_free(ctx, d_median); lvk_hip_free(ctx, d_grid); lvk_hip_free(ctx, d_keep);
        lvk_hip_free(ctx, d_range); lvk_hip_free(ctx, d_tab);
        d_small = d_median = d_grid = nullptr; d_keep = nullptr; d_range = nullptr; d_tab = nullptr;
        small_cap = median_cap = grid_cap = keep_cap = range_cap = tab_cap = 0;
    }
};

namespace deblock {

constexpr int kMaxFilterSize = 255;       // apply refuses larger windows (declared deviation)

// What one apply works on: the macroblock extent, the filter region, the small frame and the mode of the downscale
struct Geometry
{
    int bs, ex, ey, rw, rh, ws, hs;
    int iscale; bool fast; double scale;      // fast: resizeAreaFast_ by iscale; else the area tables of `scale`
};

// The two launches deblock_420.hip reuses unchanged (deblock.hip): the block statistics of a one-channel plane into d's grids (k_deblock_stats<1>,
// dwords where the plane allows) and the median of d->d_small (three channels) into d->d_median (k_deblock_median<3>)
int launch_stats_plane(lvk_hip_deblock* d, const uint8_t* plane, int step, const Geometry& g);
int launch_median_c3(lvk_hip_deblock* d, const Geometry& g);

// lvk_hip_deblock_apply_yuv420 behind its entry guard (deblock_420.hip): also the I420 / I40A / NV12 route of lvk_hip_deblock_apply_obs
// (deblock_obs.hip); `name` is the entry's
int apply_420(lvk_hip_deblock* d, const char* name, const yuv420::PlaneSet& src, const yuv420::PlaneSet& dst, int region_xywh[4]);

__device__ __forceinline__ int sat_u8(float v)           // saturate_cast<uchar>(float): round half to even, clamp
{
    const float r = rintf(v);
    return r < 0.f ? 0 : r > 255.f ? 255 : (int)r;
}

// resizeAreaFast_ of one block of bs x bs values: 2 x 2 as (sum + 2) >> 2, else sum * (1.f / area) rounded half to even
__device__ __forceinline__ int box_mean(long long sum, int bs, float inv_area)
{
    return bs == 2 ? (int)((sum + 2) >> 2) : sat_u8((float)sum * inv_area);
}

__device__ __forceinline__ int byte_of(uint32_t v, int c) { return (int)((v >> (8 * c)) & 255u); }

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The statistics of one macroblock by one wave, two passes: the exact integer block mean of the grey, then the mean absolute deviation from it, and
// keep_block = float(min(grid, L) * (1.0 / L)).  visit(f) calls f(grey) for every pixel of the block, the wave's lanes striding over it: the bytes
// of a packed frame (k_deblock_stats, deblock.hip) or the luma bytes of a packed YUV layout (k_deblock_stats_luma, deblock_obs.hip).  The second
// pass reads the same, cache-resident bytes.  o: the block's index in the three grids.
template <typename Visit>
__device__ __forceinline__ void block_stats(Visit visit, int bs, float inv_area, int levels, double level_step, int lane, size_t o,
                                            uint8_t* __restrict__ mean_out, uint8_t* __restrict__ grid_out, float* __restrict__ keep_out)
{
    long long sum = 0;
    visit([&](int g) { sum += g; });
    const int mean = box_mean(wave_sum(sum), bs, inv_area);
    long long dev = 0;                          // the block's bytes are still in L1 / L2: one HBM read for both passes
    visit([&](int g) { dev += abs(g - mean); });
    const int grid = box_mean(wave_sum(dev), bs, inv_area);
    if (lane == 0)
    {
        mean_out[o] = (uint8_t)mean;
        grid_out[o] = (uint8_t)grid;
        keep_out[o] = (float)((double)min(grid, levels) * level_step);
    }
}

template <int BPP>
__device__ __forceinline__ uint32_t load_pixel(const uint8_t* __restrict__ p)       // a pixel's channels in bytes 0 .. BPP - 1
{
    if constexpr (BPP == 4) return *reinterpret_cast<const uint32_t*>(p);
    else if constexpr (BPP == 3) return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    else return *p;
}

template <int BPP>
__device__ __forceinline__ void store_pixel(uint8_t* __restrict__ p, uint32_t v)
{
    if constexpr (BPP == 4) *reinterpret_cast<uint32_t*>(p) = v;
    else if constexpr (BPP == 3) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); }
    else *p = (uint8_t)v;
}

// One pixel (x, y) of the INTER_AREA of the region (BPP channels) to hs x ws, stored at d.  row(yy) is a handle of the region's row yy and
// px(handle, xx) its pixel xx, channels in bytes 0 .. BPP - 1: a packed frame's row pointer and bytes, or the rows of a 4:2:0 frame's planes.
// iscale > 0: integer scale (resizeAreaFast_; cells that reach past the source -- a destination size rounded up -- average what they cover,
// (float)sum / count); iscale == 0: separable area tables, float accumulation in table order (per source row the x taps, then the rows weighted
// by their beta).
template <int BPP, typename Row, typename Px>
__device__ __forceinline__ void down_pixel(Row row, Px px, uint8_t* __restrict__ d, int x, int y, int rh, int rw, int iscale, float inv_area,
                                           const int2* __restrict__ xr, const AreaTabEntry* __restrict__ xt,
                                           const int2* __restrict__ yr, const AreaTabEntry* __restrict__ yt)
{
    uint32_t out = 0;
    if (iscale > 0)
    {
        const int x0 = x * iscale, y0 = y * iscale;
        const int x1 = min(x0 + iscale, rw), y1 = min(y0 + iscale, rh);
        const bool full = x0 + iscale <= rw && y0 + iscale <= rh;
        int s[BPP] = {};
        for (int yy = y0; yy < y1; yy++)
        {
            const auto r = row(yy);
            for (int xx = x0; xx < x1; xx++)
            {
                const uint32_t v = px(r, xx);
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
        const auto r = row(ty.si);
        float b[BPP] = {};
        for (int i = 0; i < rx.y; i++)
        {
            const AreaTabEntry tx = xt[rx.x + i];
            const uint32_t v = px(r, tx.si);
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

// A pixel of the median frame (three bytes, any alignment) as ONE load: the dword at its address, whose fourth byte is the next pixel's first or,
// behind the last pixel, the slack deblock::reserve leaves behind the frame; byte_of never looks at it.
__device__ __forceinline__ uint32_t load_tap(const uint8_t* __restrict__ p) { return reinterpret_cast<const yuv420::P4*>(p)->w; }

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

// computeResizeAreaTab for a scale given by the caller (the 1 / filter_scaling downscale: scale = 1 / (double)(1.f / s), not ssize / dsize)
inline void area_tab(int ssize, int dsize, double scale, std::vector<int2>& range, std::vector<AreaTabEntry>& tab)
{
    range.assign((size_t)dsize, int2{0, 0});
    tab.clear();
    for (int dx = 0; dx < dsize; dx++)
    {
        const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        const double cell = std::min(scale, ssize - fsx1);
        int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        const int start = (int)tab.size();
        if (sx1 - fsx1 > 1e-3) tab.push_back({sx1 - 1, (float)((sx1 - fsx1) / cell)});
        for (int sx = sx1; sx < sx2; sx++) tab.push_back({sx, (float)(1.0 / cell)});
        if (fsx2 - sx2 > 1e-3) tab.push_back({sx2, (float)(std::min(std::min(fsx2 - sx2, 1.0), cell) / cell)});
        range[(size_t)dx] = int2{start, (int)tab.size() - start};
    }
}

inline int small_extent(int n, float scaling)          // saturate_cast<int>(n * (double)(1.f / s)); 0 where it does not fit an int
{
    const double v = std::rint((double)n * (double)(1.0f / scaling));
    return v >= 1.0 && v <= 2147483647.0 ? (int)v : 0;
}

inline int ensure(lvk_hip_ctx* ctx, void** p, size_t& cap, size_t bytes)
{
    if (*p && cap >= bytes) return LVK_HIP_OK;
    if (*p) { lvk_hip_free(ctx, *p); *p = nullptr; cap = 0; }
    const int rc = lvk_hip_malloc(ctx, bytes, p);
    if (rc == LVK_HIP_OK) cap = bytes;
    return rc;
}

inline int upload_area_tabs(lvk_hip_deblock* d, int rh, int rw, int hs, int ws, double scale)
{
    if (d->d_range && d->tab_rh == rh && d->tab_rw == rw && d->tab_hs == hs && d->tab_ws == ws && d->tab_scale == scale) return LVK_HIP_OK;
    std::vector<int2> xr, yr; std::vector<AreaTabEntry> xt, yt;
    area_tab(rw, ws, scale, xr, xt);
    area_tab(rh, hs, scale, yr, yt);
    // one block: x ranges | y ranges, and one: x taps | y taps (each range indexes its own axis' taps)
    std::vector<int2> ranges(xr); ranges.insert(ranges.end(), yr.begin(), yr.end());
    std::vector<AreaTabEntry> taps(xt); taps.insert(taps.end(), yt.begin(), yt.end());
    int rc;
    if ((rc = ensure(d->ctx, (void**)&d->d_range, d->range_cap, ranges.size() * sizeof(int2))) != LVK_HIP_OK) return rc;
    if ((rc = ensure(d->ctx, (void**)&d->d_tab, d->tab_cap, std::max<size_t>(taps.size(), 1) * sizeof(AreaTabEntry))) != LVK_HIP_OK) return rc;
    // (synchronous, once per geometry -- like the context's INTER_LINEAR / INTER_AREA table caches; the host vectors die with this call)
    LVK_HIP_CHECK(d->ctx, hipStreamSynchronize(d->ctx->stream));
    LVK_HIP_CHECK(d->ctx, hipMemcpy(d->d_range, ranges.data(), ranges.size() * sizeof(int2), hipMemcpyHostToDevice));
    if (!taps.empty()) LVK_HIP_CHECK(d->ctx, hipMemcpy(d->d_tab, taps.data(), taps.size() * sizeof(AreaTabEntry), hipMemcpyHostToDevice));
    d->d_xr = d->d_range; d->d_yr = d->d_range + xr.size();
    d->d_xt = d->d_tab; d->d_yt = d->d_tab + xt.size();
    d->tab_rh = rh; d->tab_rw = rw; d->tab_hs = hs; d->tab_ws = ws; d->tab_scale = scale;
    return LVK_HIP_OK;
}

// The geometry of an apply of settings `s` to a rows x cols frame, or the refusal of the entry `name` (nothing has changed by then)
inline int geometry(lvk_hip_ctx* ctx, const lvk_deblock_settings& s, int rows, int cols, const std::string& name, Geometry& g)
{
    LVK_HIP_REQUIRE(ctx, s.filter_size <= (uint32_t)kMaxFilterSize);
    g.bs = s.block_size > (uint32_t)std::max(rows, cols) ? 0 : (int)s.block_size;
    g.ex = g.bs ? cols / g.bs : 0; g.ey = g.bs ? rows / g.bs : 0;
    if (g.ex == 0 || g.ey == 0) return ctx->fail(LVK_HIP_ERR_ARG, name + ": the frame holds no whole macroblock (cv::resize of an empty region)");
    g.rw = g.ex * g.bs; g.rh = g.ey * g.bs;
    g.ws = small_extent(g.rw, s.filter_scaling); g.hs = small_extent(g.rh, s.filter_scaling);
    if (g.ws == 0 || g.hs == 0) return ctx->fail(LVK_HIP_ERR_ARG, name + ": the 1 / filter_scaling downscale of the region is empty");
    // downscale mode: resizeAreaFast_ when 1 / (double)(1.f / s) is an integer, else the area tables of that scale
    g.scale = 1.0 / (double)(1.0f / s.filter_scaling);
    g.iscale = (int)std::lrint(g.scale);
    g.fast = std::fabs(g.scale - g.iscale) < 2.220446049250313e-16;
    return LVK_HIP_OK;
}

// The handle's buffers for geometry `g` and `bpp` bytes per pixel of the small frame, and the area tables where the downscale needs them
inline int reserve(lvk_hip_deblock* d, const Geometry& g, int bpp)
{
    lvk_hip_ctx* ctx = d->ctx;
    int rc;
    const size_t sb = (size_t)g.hs * g.ws * bpp, cells = (size_t)g.ey * g.ex;
    if ((rc = ensure(ctx, (void**)&d->d_small, d->small_cap, sb)) != LVK_HIP_OK) return rc;
    if ((rc = ensure(ctx, (void**)&d->d_median, d->median_cap, sb + 4)) != LVK_HIP_OK) return rc;      // + 4: k_deblock_blend_420 loads a pixel as a dword
    if ((rc = ensure(ctx, (void**)&d->d_grid, d->grid_cap, cells * 2)) != LVK_HIP_OK) return rc;
    if ((rc = ensure(ctx, (void**)&d->d_keep, d->keep_cap, cells * sizeof(float))) != LVK_HIP_OK) return rc;
    if (!g.fast && (rc = upload_area_tabs(d, g.rh, g.rw, g.hs, g.ws, g.scale)) != LVK_HIP_OK) return rc;
    return LVK_HIP_OK;
}

// The tables of the blend for the geometry the handle holds: `keep` (float bilinear of keep_block) and `smooth` (8U bilinear of the median frame)
inline int blend_tables(lvk_hip_ctx* ctx, const lvk_hip_deblock* d, bool smooth, const LinTabEntry** kx, const LinTabEntry** ky,
                        const Lin8Entry** sx, const Lin8Entry** sy)
{
    int rc;
    if ((rc = lvk_get_lintab(ctx, d->ex, d->rw, false, kx)) != LVK_HIP_OK) return rc;
    if ((rc = lvk_get_lintab(ctx, d->ey, d->rh, true, ky)) != LVK_HIP_OK) return rc;
    if (smooth)
    {
        if ((rc = lvk_get_lin8tab(ctx, d->ws, d->rw, false, sx)) != LVK_HIP_OK) return rc;
        if ((rc = lvk_get_lin8tab(ctx, d->hs, d->rh, true, sy)) != LVK_HIP_OK) return rc;
    }
    return LVK_HIP_OK;
}

} // namespace deblock
