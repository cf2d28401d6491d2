// The packed source of the sharpening kernels that write a format's planes (k_rcas_420 of scaling_420.hip, k_rcas_obs of scaling_obs.hip): the rows of a
// packed 8UC3 frame as a thread of four columns x ROWS rows reads them, on top of rcas_core.hpp.  Written once, included by both units; the names of
// rcas_core.hpp are qualified because scaling_obs.hip also includes remap_core.hpp, which has helpers of the same names.
#pragma once

#include "rcas_core.hpp"

namespace {

constexpr int ROWS = 4;                                   // rows per thread, as lvk_launch_sharpen chose them

// Rows of a packed 8UC3 frame, loaded as k_rcas loads them.  A thread at the right edge that has fewer than four columns (cols % 4 != 0) has no 12 bytes
// of its own: it reads its six pixels one by one, columns clamped into the row.
struct PackedSrc
{
    const uint8_t* src; int step;
    struct Raw { rcas::RawRow r[ROWS + 2]; };

    __device__ __forceinline__ void load(Raw& raw, int x0, int y0, int rows, int cols, int) const
    {
        if (x0 + rcas::RCAS_PXT <= cols)
        {
#pragma unroll
            for (int r = 0; r < ROWS + 2; r++) raw.r[r] = rcas::load_row(src, step, y0 - 1 + r, rows, x0, cols);
            return;
        }
#pragma unroll
        for (int r = 0; r < ROWS + 2; r++)
        {
            const uint8_t* rp = src + (long)min(max(y0 - 1 + r, 0), rows - 1) * step;
            uint32_t p[rcas::RCAS_PXT + 2];
#pragma unroll
            for (int j = 0; j < rcas::RCAS_PXT + 2; j++) p[j] = rcas::load_px_raw(rp + 3 * (long)min(max(x0 - 1 + j, 0), cols - 1));
            raw.r[r] = rcas::RawRow{p[1] | (p[2] << 24), (p[2] >> 8) | (p[3] << 16), (p[3] >> 16) | (p[4] << 8), p[0], p[5]};
        }
    }
    __device__ __forceinline__ rcas::Row row(const Raw& raw, int r) const { return rcas::unpack_row(raw.r[r]); }
    __device__ __forceinline__ void centre(const Raw& raw, int r, uint32_t (&c)[rcas::RCAS_PXT]) const
    {
        const rcas::RawRow& m = raw.r[r];
        c[0] = m.w0 & 0xffffffu; c[1] = (m.w0 >> 24) | ((m.w1 & 0xffffu) << 8); c[2] = (m.w1 >> 16) | ((m.w2 & 0xffu) << 16); c[3] = m.w2 >> 8;
    }
};

} // namespace
