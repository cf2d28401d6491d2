// The CAS filter (cas.hip) on ONE-channel frames (8UC1, VideoFrame::GRAY) for gfx950: the kernel behind lvk_hip_cas_gray.
//
// The plugin runs CAS as an RGBA effect, so there is no one-channel program to copy.  DEFINITION: channel 0 of the
// three-channel specification (tests/np_cas.py) on (g, g, g).  CAS sharpens every channel on its own, so that is cas_channel of cas_core.hpp,
// the very function k_cas<C> calls three times per pixel, called once: load u / 255 correctly rounded, neighbours outside the frame read as 0,
// store rint(v * 255).  Out of place.
//
// Shape: that of k_rcas_px<GrayRcas> (sharpen_px.hip), which has the same 3 x 3 footprint.  No LDS.  A thread owns kPxt adjacent pixels of kRows
// rows: it loads the kRows + 2 source rows it needs at once -- per row one (unaligned) dword that lies inside the row plus the byte on either
// side -- converts each byte once and walks the rows with a rolling three-row window in registers.  Its four results of a row leave as one dword.
// The groups of a wave's rows are shifted left by the misalignment of their first destination row (0 .. 3 pixels), so that with a pitch that
// keeps the rows aligned alike every store is aligned whatever the base address is; a destination row that is not dword-aligned (odd pitches)
// leaves as bytes.  The first and the last group of a row, where the frame ends inside the group, go pixel by pixel.  No load touches a byte
// outside the cols bytes of a frame row (a side or a row beyond the frame is loaded from a clamped in-frame address and replaced by 0), and only
// the cols bytes of a destination row are written.
#include "lvk_hip_internal.hpp"
#include "cas_core.hpp"

#include <algorithm>
#include <cstdint>

namespace {

using namespace ffx;

constexpr int kPxt = 4;                    // pixels per thread and row: one dword
constexpr int kStripW = 64 * kPxt;         // pixels per wave and row
constexpr int kRows = 4;                   // rows per thread
constexpr int kBlockH = 4 * kRows;         // rows per block: one band of kRows rows per wave

struct __attribute__((packed, aligned(1))) GrayWord { uint32_t w; };          // four GRAY pixels at any address

// the texel at (x, y) as CAS sees it: 0 outside the frame
__device__ __forceinline__ float texel_or_zero(const uint8_t* __restrict__ src, long long src_step, int rows, int cols, int x, int y)
{
    if (x < 0 || x >= cols || y < 0 || y >= rows) return 0.0f;
    return unit_of((float)src[(long long)y * src_step + x]);
}

__global__ __launch_bounds__(256)
void k_cas_gray(const uint8_t* __restrict__ src, long long src_step, int rows, int cols, uint8_t* __restrict__ dst, long long dst_step, float peak)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int y0 = ((int)blockIdx.y * 4 + wave) * kRows; y0 < rows; y0 += (int)gridDim.y * kBlockH)
    {
        // pixels by which the band's first destination row lies past a dword boundary (wave-uniform)
        const int mis = (int)(reinterpret_cast<uintptr_t>(dst + (long long)y0 * dst_step) & 3u);
        const int x0 = (int)blockIdx.x * kStripW + lane * kPxt - mis;
        if (x0 >= cols) continue;                                        // (x0 + kPxt > 0 always: mis <= 3)
        const int y1 = min(y0 + kRows, rows);

        if (x0 < 0 || x0 + kPxt > cols)                                  // the frame ends inside the group: one pixel at a time
        {
            for (int y = y0; y < y1; y++)
                for (int x = max(x0, 0); x < min(x0 + kPxt, cols); x++)
                {
                    float n[3][3];
#pragma unroll
                    for (int dy = 0; dy < 3; dy++)
#pragma unroll
                        for (int dx = 0; dx < 3; dx++) n[dy][dx] = texel_or_zero(src, src_step, rows, cols, x + dx - 1, y + dy - 1);
                    const float v = cas_channel(n[0][0], n[0][1], n[0][2], n[1][0], n[1][1], n[1][2], n[2][0], n[2][1], n[2][2], peak);
                    dst[(long long)y * dst_step + x] = (uint8_t)to_byte(v);
                }
            continue;
        }

        // Unconditional loads (no branches, so that all rows of a thread are in flight together) from addresses clamped into the frame: a row
        // above or below the frame and a side beyond it are loaded from their in-frame neighbour and zeroed below.  0 <= x0, x0 + kPxt <= cols.
        const bool has_left = x0 > 0, has_right = x0 + kPxt < cols;
        uint32_t word[kRows + 2], left[kRows + 2], right[kRows + 2];     // rows y0 - 1 .. y0 + kRows
#pragma unroll
        for (int r = 0; r < kRows + 2; r++)
        {
            const uint8_t* rp = src + (long long)min(max(y0 - 1 + r, 0), rows - 1) * src_step + x0;
            word[r] = reinterpret_cast<const GrayWord*>(rp)->w;
            left[r] = *(has_left ? rp - 1 : rp);
            right[r] = *(has_right ? rp + kPxt : rp + kPxt - 1);
        }
        float win[3][kPxt + 2];                                          // the rolling window: pixels x0 - 1 .. x0 + kPxt of three rows
        auto unpack = [&](int r, float (&o)[kPxt + 2]) {
            const int y = y0 - 1 + r;
            const bool in = y >= 0 && y < rows;
            o[0] = in && has_left ? unit_of((float)left[r]) : 0.0f;
#pragma unroll
            for (int p = 0; p < kPxt; p++)
            {
                const float v = unit_of((float)((word[r] >> (8 * p)) & 0xffu));
                o[p + 1] = in ? v : 0.0f;
            }
            o[kPxt + 1] = in && has_right ? unit_of((float)right[r]) : 0.0f;
        };
        unpack(0, win[0]);
        unpack(1, win[1]);
#pragma unroll
        for (int r = 0; r < kRows; r++)
        {
            const int y = y0 + r;
            if (y >= rows) break;
            const float (&up)[kPxt + 2] = win[r % 3];
            const float (&mid)[kPxt + 2] = win[(r + 1) % 3];
            float (&down)[kPxt + 2] = win[(r + 2) % 3];
            unpack(r + 2, down);
            uint32_t out[kPxt];
#pragma unroll
            for (int p = 0; p < kPxt; p++)
                out[p] = to_byte(cas_channel(up[p], up[p + 1], up[p + 2], mid[p], mid[p + 1], mid[p + 2], down[p], down[p + 1], down[p + 2], peak));
            uint8_t* q = dst + (long long)y * dst_step + x0;
            if ((reinterpret_cast<uintptr_t>(q) & 3u) == 0) *reinterpret_cast<uint32_t*>(q) = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
            else
#pragma unroll
                for (int p = 0; p < kPxt; p++) q[p] = (uint8_t)out[p];
        }
    }
}

} // namespace

extern "C" {

int lvk_hip_cas_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step, float sharpness)
{
    LVK_HIP_ENTRY(ctx);
    if (!(sharpness >= 0.0f && sharpness <= 1.0f)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_cas_gray: sharpness must lie in [0, 1] (CASFilter.cpp)");
    LVK_HIP_REQUIRE(ctx, d_src && d_dst && rows > 0 && cols > 0);
    LVK_HIP_REQUIRE(ctx, src_step >= cols && dst_step >= cols);
    // CAS reads its neighbours: a destination that overlaps the source (in place included) would race
    if (lvk_pitched_overlap(d_src, src_step, rows, cols, d_dst, dst_step, rows, cols)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_cas_gray: the source and destination overlap");
    float peak = 0.0f;
    lvk_hip_cas_const(sharpness, &peak);

    // (cols + 3: the 0 .. 3 pixels a misaligned destination row shifts its groups by)
    const unsigned gx = (unsigned)(((long long)cols + 3 + kStripW - 1) / kStripW);
    const unsigned gy = (unsigned)std::min<long long>(((long long)rows + kBlockH - 1) / kBlockH, 65535);
    hipLaunchKernelGGL(k_cas_gray, dim3(gx, gy), dim3(256), 0, ctx->stream, (const uint8_t*)d_src, (long long)src_step, rows, cols, (uint8_t*)d_dst,
                       (long long)dst_step, peak);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

} // extern "C"
