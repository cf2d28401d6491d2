// Host side of lvk::DeblockingFilter shared by its translation units: deblock.hip (packed 8UC3 frames, the handle's entry points) and
// deblock_px.hip (one- and four-channel frames).  The handle, the geometry rules of an apply and the area tables of the non-integer
// downscale are independent of the pixel size; the kernels are not and stay with their unit.
#pragma once

#include "lvk_hip_internal.hpp"

#include <cmath>
#include <algorithm>
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

namespace lvk_deblock {

constexpr int kMaxFilterSize = 255;       // apply refuses larger windows (declared deviation)
constexpr int kMedTile = 16;              // median: 16 x 16 outputs per block
constexpr int kMedLdsMaxK = 113;          // (16 + k - 1)^2 packed pixels fit 64 KiB of LDS up to this k; larger k read global memory

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

} // namespace lvk_deblock
