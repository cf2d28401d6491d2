// Debug overlays of the stabilization filter for gfx950: the motion-mesh grid and the tracker
// crosses the OBS plugin's test mode draws into the newest queued frame, and the test-mode HUD: points,
// rectangles and text, drawn on the device where the reference maps the frame to the host for cv::rectangle / cv::putText.
//
// Replaces lvk::draw_grid / lvk::draw_crosses (reference: LiveVisionKit/Functions/Drawing.tpp:53-93,146-196) and their
// kernels `grid` / `crosses` (Functions/OpenCL/Sources/Drawing.cl:22-39,75-105), plus StabilizationFilter::draw_trackers /
// draw_motion_mesh (Filters/StabilizationFilter.cpp:163-188) and FrameTracker::draw_trackers (Vision/FrameTracker.cpp:489-505).
// lvk::draw_points and its kernel `points` (Drawing.tpp:95-141, Drawing.cl:43-69); lvk::draw_rect / lvk::draw_text (Drawing.tpp:40-49,198-218;
// VSFilter::draw_debug_hud, Sources/Stabilisation/VSFilter.cpp:368-383).  Specification of the last three: tests/np_draw.py.
// Pure integer / exact-fmod work, byte stores only where a drawn pixel lies.
#include "lvk_hip_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

// Drawing.cl:22-39.  One thread per pixel of a row segment; only line pixels are written.
__global__ __launch_bounds__(256)
void k_draw_grid(uint8_t* __restrict__ dst, int dst_step, int rows, int cols, float cell_w, float cell_h, int thickness, uint32_t colour)
{
    const int x = (int)(blockIdx.x * 64 + threadIdx.x), y = (int)(blockIdx.y * 4 + threadIdx.y);
    if (x >= cols || y >= rows) return;
    const float fx = fmodf((float)x, cell_w), fy = fmodf((float)y, cell_h);        // exact by definition
    const float t = (float)thickness;
    if (fx < t || fy < t || fx > cell_w - t - 1.0f || fy > cell_h - t - 1.0f)
    {
        uint8_t* d = dst + (long)y * dst_step + 3 * x;
        d[0] = (uint8_t)colour; d[1] = (uint8_t)(colour >> 8); d[2] = (uint8_t)(colour >> 16);
    }
}

// Drawing.cl:75-105.  One thread per point; overlapping crosses store the same colour, so the store order is immaterial.
__global__ __launch_bounds__(64)
void k_draw_crosses(const int2* __restrict__ pts, int n, uint8_t* __restrict__ dst, int dst_step, int rows, int cols,
                    int cross_size, int thickness, uint32_t colour)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int2 c = pts[i];
    // the sums below cannot overflow: the host clamps coordinates to +-2^30
    int x = max(c.x - cross_size, 0), y = max(c.y - cross_size, 0);
    const int max_x = min(c.x + cross_size + 1, cols - thickness), max_y = min(c.y + cross_size + 1, rows - thickness);
    const uint8_t c0 = (uint8_t)colour, c1 = (uint8_t)(colour >> 8), c2 = (uint8_t)(colour >> 16);
    for (int k = 1; x < max_x && y < max_y; k++)
    {
        for (int dx = 0; dx < thickness; dx++)
        {
            uint8_t* f = dst + (long)y * dst_step + 3 * (x + dx);
            f[0] = c0; f[1] = c1; f[2] = c2;
            uint8_t* b = dst + (long)y * dst_step + 3 * (max_x - k + dx);
            b[0] = c0; b[1] = c1; b[2] = c2;
        }
        x++; y++;
    }
}

// Drawing.cl:43-69.  One thread per point: the square [px - half, px + half) x [py - half, py + half) clipped to the frame (64-bit sums:
// half may be anything up to 2^30).
__global__ __launch_bounds__(64)
void k_draw_points(const int2* __restrict__ pts, int n, uint8_t* __restrict__ dst, int dst_step, int rows, int cols, int half, uint32_t colour)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int2 c = pts[i];
    const int min_x = (int)max((long long)c.x - half, 0LL), min_y = (int)max((long long)c.y - half, 0LL);
    const int max_x = (int)min((long long)c.x + half, (long long)cols), max_y = (int)min((long long)c.y + half, (long long)rows);
    const uint8_t c0 = (uint8_t)colour, c1 = (uint8_t)(colour >> 8), c2 = (uint8_t)(colour >> 16);
    for (int y = min_y; y < max_y; y++)
        for (int x = min_x; x < max_x; x++)
        {
            uint8_t* d = dst + (long)y * dst_step + 3 * x;
            d[0] = c0; d[1] = c1; d[2] = c2;
        }
}

// The pixels of a rectangle's band, already clipped to the frame by the host: `full` whole rows of the box [x0, x0 + w) -- the first `top`
// of them from row y0 down, the others from row bottom_y0 -- and then, between them, `side` pixels a row from row mid_y0: `left` from
// x0 and the rest from right_x0.  A filled rectangle, or a band whose hole is not in the frame, is whole rows only.
struct RectSpans
{
    int x0, y0, w, top, bottom_y0, mid_y0, left, right_x0, side;
    uint32_t full_px, total_px;              // full * w; full_px + middle rows * side
};

// One thread per band pixel, none for the hole: a 1080p HUD outline is about 9 600 threads, not the 1.3 million of its bounding box.
__global__ __launch_bounds__(256)
void k_draw_rect(uint8_t* __restrict__ dst, int dst_step, RectSpans s, uint32_t colour)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= s.total_px) return;
    int x, y;
    if (i < s.full_px)
    {
        const uint32_t r = i / (uint32_t)s.w, c = i - r * (uint32_t)s.w;
        y = (int)r < s.top ? s.y0 + (int)r : s.bottom_y0 + ((int)r - s.top);
        x = s.x0 + (int)c;
    }
    else
    {
        const uint32_t j = i - s.full_px, r = j / (uint32_t)s.side, c = j - r * (uint32_t)s.side;
        y = s.mid_y0 + (int)r;
        x = (int)c < s.left ? s.x0 + (int)c : s.right_x0 + ((int)c - s.left);
    }
    uint8_t* d = dst + (long)y * dst_step + 3 * x;
    d[0] = (uint8_t)colour; d[1] = (uint8_t)(colour >> 8); d[2] = (uint8_t)(colour >> 16);
}

// The font of lvk_hip_draw_text: this project's own 5 x 7 glyphs for printable ASCII 0x20 .. 0x7E, one byte a row, top row first, bit 4 the
// left column.  NOT OpenCV's Hershey glyphs.  tests/np_draw.py draws the same table as text; the GPU suite renders every glyph through both.
constexpr int kGlyphW = 5, kGlyphH = 7, kCellW = 6, kFirstGlyph = 0x20, kGlyphs = 95;
__constant__ uint8_t kFont[kGlyphs][kGlyphH] = {
    {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00}, {0x04, 0x04, 0x04, 0x04, 0x04, 0x00, 0x04}, {0x0A, 0x0A, 0x0A, 0x00, 0x00, 0x00, 0x00}, {0x0A, 0x0A, 0x1F, 0x0A, 0x1F, 0x0A, 0x0A},   //   ! " #
    {0x04, 0x0F, 0x14, 0x0E, 0x05, 0x1E, 0x04}, {0x18, 0x19, 0x02, 0x04, 0x08, 0x13, 0x03}, {0x0C, 0x12, 0x14, 0x08, 0x15, 0x12, 0x0D}, {0x04, 0x04, 0x04, 0x00, 0x00, 0x00, 0x00},   // $ % & '
    {0x06, 0x08, 0x10, 0x10, 0x10, 0x08, 0x06}, {0x0C, 0x02, 0x01, 0x01, 0x01, 0x02, 0x0C}, {0x00, 0x04, 0x15, 0x0E, 0x15, 0x04, 0x00}, {0x00, 0x04, 0x04, 0x1F, 0x04, 0x04, 0x00},   // ( ) * +
    {0x00, 0x00, 0x00, 0x00, 0x0C, 0x04, 0x08}, {0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00}, {0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C}, {0x00, 0x01, 0x02, 0x04, 0x08, 0x10, 0x00},   // , - . /
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E}, {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F}, {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E},   // 0 1 2 3
    {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E}, {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08},   // 4 5 6 7
    {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E}, {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}, {0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x0C, 0x00}, {0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x04, 0x08},   // 8 9 : ;
    {0x02, 0x04, 0x08, 0x10, 0x08, 0x04, 0x02}, {0x00, 0x00, 0x1F, 0x00, 0x1F, 0x00, 0x00}, {0x08, 0x04, 0x02, 0x01, 0x02, 0x04, 0x08}, {0x0E, 0x11, 0x01, 0x02, 0x04, 0x00, 0x04},   // < = > ?
    {0x0E, 0x11, 0x01, 0x0D, 0x15, 0x15, 0x0E}, {0x0E, 0x11, 0x11, 0x11, 0x1F, 0x11, 0x11}, {0x1E, 0x11, 0x11, 0x1E, 0x11, 0x11, 0x1E}, {0x0E, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0E},   // @ A B C
    {0x1C, 0x12, 0x11, 0x11, 0x11, 0x12, 0x1C}, {0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x1F}, {0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x10}, {0x0E, 0x11, 0x10, 0x17, 0x11, 0x11, 0x0F},   // D E F G
    {0x11, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11}, {0x0E, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E}, {0x07, 0x02, 0x02, 0x02, 0x02, 0x12, 0x0C}, {0x11, 0x12, 0x14, 0x18, 0x14, 0x12, 0x11},   // H I J K
    {0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x1F}, {0x11, 0x1B, 0x15, 0x15, 0x11, 0x11, 0x11}, {0x11, 0x11, 0x19, 0x15, 0x13, 0x11, 0x11}, {0x0E, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E},   // L M N O
    {0x1E, 0x11, 0x11, 0x1E, 0x10, 0x10, 0x10}, {0x0E, 0x11, 0x11, 0x11, 0x15, 0x12, 0x0D}, {0x1E, 0x11, 0x11, 0x1E, 0x14, 0x12, 0x11}, {0x0F, 0x10, 0x10, 0x0E, 0x01, 0x01, 0x1E},   // P Q R S
    {0x1F, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04}, {0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E}, {0x11, 0x11, 0x11, 0x11, 0x11, 0x0A, 0x04}, {0x11, 0x11, 0x11, 0x15, 0x15, 0x15, 0x0A},   // T U V W
    {0x11, 0x11, 0x0A, 0x04, 0x0A, 0x11, 0x11}, {0x11, 0x11, 0x11, 0x0A, 0x04, 0x04, 0x04}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x10, 0x1F}, {0x0E, 0x08, 0x08, 0x08, 0x08, 0x08, 0x0E},   // X Y Z [
    {0x00, 0x10, 0x08, 0x04, 0x02, 0x01, 0x00}, {0x0E, 0x02, 0x02, 0x02, 0x02, 0x02, 0x0E}, {0x04, 0x0A, 0x11, 0x00, 0x00, 0x00, 0x00}, {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x1F},   // backslash ] ^ _
    {0x08, 0x04, 0x02, 0x00, 0x00, 0x00, 0x00}, {0x00, 0x00, 0x0E, 0x01, 0x0F, 0x11, 0x0F}, {0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x1E}, {0x00, 0x00, 0x0E, 0x10, 0x10, 0x11, 0x0E},   // ` a b c
    {0x01, 0x01, 0x0D, 0x13, 0x11, 0x11, 0x0F}, {0x00, 0x00, 0x0E, 0x11, 0x1F, 0x10, 0x0E}, {0x06, 0x09, 0x08, 0x1C, 0x08, 0x08, 0x08}, {0x00, 0x0F, 0x11, 0x11, 0x0F, 0x01, 0x0E},   // d e f g
    {0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x11}, {0x04, 0x00, 0x0C, 0x04, 0x04, 0x04, 0x0E}, {0x02, 0x00, 0x06, 0x02, 0x02, 0x12, 0x0C}, {0x10, 0x10, 0x12, 0x14, 0x18, 0x14, 0x12},   // h i j k
    {0x0C, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E}, {0x00, 0x00, 0x1A, 0x15, 0x15, 0x11, 0x11}, {0x00, 0x00, 0x16, 0x19, 0x11, 0x11, 0x11}, {0x00, 0x00, 0x0E, 0x11, 0x11, 0x11, 0x0E},   // l m n o
    {0x00, 0x1E, 0x11, 0x11, 0x1E, 0x10, 0x10}, {0x00, 0x0F, 0x11, 0x11, 0x0F, 0x01, 0x01}, {0x00, 0x00, 0x16, 0x19, 0x10, 0x10, 0x10}, {0x00, 0x00, 0x0E, 0x10, 0x0E, 0x01, 0x1E},   // p q r s
    {0x08, 0x08, 0x1C, 0x08, 0x08, 0x09, 0x06}, {0x00, 0x00, 0x11, 0x11, 0x11, 0x13, 0x0D}, {0x00, 0x00, 0x11, 0x11, 0x11, 0x0A, 0x04}, {0x00, 0x00, 0x11, 0x11, 0x15, 0x15, 0x0A},   // t u v w
    {0x00, 0x00, 0x11, 0x0A, 0x04, 0x0A, 0x11}, {0x00, 0x11, 0x11, 0x11, 0x0F, 0x01, 0x0E}, {0x00, 0x00, 0x1F, 0x02, 0x04, 0x08, 0x1F}, {0x02, 0x04, 0x04, 0x08, 0x04, 0x04, 0x02},   // x y z {
    {0x04, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04}, {0x08, 0x04, 0x04, 0x02, 0x04, 0x04, 0x08}, {0x00, 0x00, 0x08, 0x15, 0x02, 0x00, 0x00},   // | } ~
};

__device__ __forceinline__ int floor_div(int a, int b) { return a >= 0 ? a / b : -((b - 1 - a) / b); }      // b > 0

// One launch per string: a thread per pixel of the text's box, clipped to the frame at (x0, y0), w x h.  (u, v) is the pixel relative to
// the top-left corner of the first glyph.  Font pixel (k, r) -- column k = 6 i + c of the string -- is the block [k s, k s + s) x
// [r s, r s + s) grown by g on each side, so the pixel is set iff a set font pixel lies in [(u - g) / s, (u + g) / s] x [(v - g) / s, (v + g) / s].
__global__ __launch_bounds__(256)
void k_draw_text(const uint8_t* __restrict__ text, int n, uint8_t* __restrict__ dst, int dst_step, int x0, int y0, int w, int h, int u0, int v0,
                 int s, int g, uint32_t colour)
{
    const int ix = (int)(blockIdx.x * 64 + threadIdx.x), iy = (int)(blockIdx.y * 4 + threadIdx.y);
    if (ix >= w || iy >= h) return;
    const int u = u0 + ix, v = v0 + iy;
    const int k0 = max(floor_div(u - g, s), 0), k1 = min(floor_div(u + g, s), kCellW * n - 1);
    const int r0 = max(floor_div(v - g, s), 0), r1 = min(floor_div(v + g, s), kGlyphH - 1);
    bool hit = false;
    for (int k = k0; k <= k1 && !hit; k++)
    {
        const int i = k / kCellW, c = k - kCellW * i;
        if (c >= kGlyphW) continue;                                            // the blank column between two glyphs
        const unsigned byte = text[i], glyph = byte - kFirstGlyph < (unsigned)kGlyphs ? byte - kFirstGlyph : '?' - kFirstGlyph;
        for (int r = r0; r <= r1; r++) hit |= (kFont[glyph][r] >> (kGlyphW - 1 - c)) & 1;
    }
    if (!hit) return;
    uint8_t* d = dst + (long)(y0 + iy) * dst_step + 3 * (x0 + ix);
    d[0] = (uint8_t)colour; d[1] = (uint8_t)(colour >> 8); d[2] = (uint8_t)(colour >> 16);
}

inline uint32_t pack3(const uint8_t c[3]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }

// The point upload of lvk::draw_crosses and lvk::draw_points: n (x, y) floats on the HOST, scaled like cv::multiply(points, Scalar(sx, sy),
// CV_32S) on 32F data -- binary32 product, round half to even, saturate (Drawing.tpp:117-120,170-173) -- and staged on the device.
int stage_points(lvk_hip_ctx* ctx, hipStream_t stream, const float* pts, int n, float scale_x, float scale_y, void** d_pts)
{
    LVK_HIP_REQUIRE(ctx, (size_t)n * sizeof(int2) <= lvk_hip_ctx::kStageBytes);
    std::vector<int2> ip((size_t)n);
    auto to_int = [](float v) -> int {
        if (!(v == v)) return 0;
        const float r = std::nearbyintf(v);                                  // FE_TONEAREST: half to even
        const float lim = 1073741824.0f;                                     // keeps the kernels' +- size sums in range
        return (int)std::fmin(std::fmax(r, -lim), lim);
    };
    for (int i = 0; i < n; i++) ip[(size_t)i] = make_int2(to_int(pts[2 * i] * scale_x), to_int(pts[2 * i + 1] * scale_y));
    return lvk_stage_params(ctx, stream, ip.data(), ip.size() * sizeof(int2), d_pts);
}

} // namespace

int lvk_launch_draw_grid(lvk_hip_ctx* ctx, hipStream_t stream, void* d_dst, int dst_step, int rows, int cols, int grid_w, int grid_h,
                         const uint8_t colour[3], int thickness)
{
    LVK_HIP_REQUIRE(ctx, d_dst && rows > 0 && cols > 0 && dst_step >= 3 * cols && colour);                  // Drawing.tpp:60-62
    LVK_HIP_REQUIRE(ctx, thickness >= 1 && grid_w >= 1 && grid_h >= 1);
    const float cw = (float)cols / (float)grid_w, ch = (float)rows / (float)grid_h;                       // Drawing.tpp:70-71
    hipLaunchKernelGGL(k_draw_grid, dim3((unsigned)((cols + 63) / 64), (unsigned)((rows + 3) / 4)), dim3(64, 4), 0, stream,
                       (uint8_t*)d_dst, dst_step, rows, cols, cw, ch, thickness, pack3(colour));
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// pts: n (x, y) floats on the HOST (stage_points)
int lvk_launch_draw_crosses(lvk_hip_ctx* ctx, hipStream_t stream, void* d_dst, int dst_step, int rows, int cols, const float* pts, int n,
                            float scale_x, float scale_y, const uint8_t colour[3], int cross_size, int thickness)
{
    LVK_HIP_REQUIRE(ctx, d_dst && rows > 0 && cols > 0 && dst_step >= 3 * cols && colour && (pts || n == 0) && n >= 0);
    LVK_HIP_REQUIRE(ctx, scale_x >= 0 && scale_y >= 0 && thickness >= 1 && cross_size >= 1);                // Drawing.tpp:155-159
    if (n == 0) return LVK_HIP_OK;                                                                         // Drawing.tpp:161-162
    void* d_pts = nullptr;
    int rc = stage_points(ctx, stream, pts, n, scale_x, scale_y, &d_pts);
    if (rc != LVK_HIP_OK) return rc;
    hipLaunchKernelGGL(k_draw_crosses, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, (const int2*)d_pts, n, (uint8_t*)d_dst, dst_step, rows, cols,
                       (cross_size + 1) / 2, thickness, pack3(colour));                                  // Drawing.tpp:183
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// Drawing.tpp:95-141
static int launch_draw_points(lvk_hip_ctx* ctx, hipStream_t stream, void* d_dst, int dst_step, int rows, int cols, const float* pts, int n,
                              float scale_x, float scale_y, const uint8_t colour[3], int point_size)
{
    LVK_HIP_REQUIRE(ctx, d_dst && rows > 0 && cols > 0 && dst_step >= 3 * cols && colour && (pts || n == 0) && n >= 0);
    LVK_HIP_REQUIRE(ctx, scale_x >= 0 && scale_y >= 0 && point_size >= 1);                                  // Drawing.tpp:104-107
    if (n == 0) return LVK_HIP_OK;                                                                         // Drawing.tpp:109-110
    void* d_pts = nullptr;
    int rc = stage_points(ctx, stream, pts, n, scale_x, scale_y, &d_pts);
    if (rc != LVK_HIP_OK) return rc;
    hipLaunchKernelGGL(k_draw_points, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, (const int2*)d_pts, n, (uint8_t*)d_dst, dst_step, rows, cols,
                       point_size / 2 + point_size % 2, pack3(colour));                                   // Drawing.tpp:130
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// cv::rectangle(dst, Rect, colour, thickness) with square corners (tests/np_draw.py rect_mask).  64-bit on the host, so no x + w overflows.
static int launch_draw_rect(lvk_hip_ctx* ctx, hipStream_t stream, void* d_dst, int dst_step, int rows, int cols, const int rect[4],
                            const uint8_t colour[3], int thickness)
{
    LVK_HIP_REQUIRE(ctx, d_dst && rows > 0 && cols > 0 && dst_step >= 3 * cols && colour && rect);
    LVK_HIP_REQUIRE(ctx, thickness != 0 && rect[2] > 0 && rect[3] > 0);
    const bool fill = thickness < 0;
    const long a = fill ? 0 : thickness / 2, b = fill ? 0 : (thickness - 1) / 2;
    const long x0 = rect[0], y0 = rect[1], x1 = x0 + rect[2] - 1, y1 = y0 + rect[3] - 1;
    // the band's outer box, clipped to the frame (inclusive)
    const long cx0 = std::max(x0 - a, 0L), cy0 = std::max(y0 - a, 0L), cx1 = std::min(x1 + b, (long)cols - 1), cy1 = std::min(y1 + b, (long)rows - 1);
    if (cx0 > cx1 || cy0 > cy1) return LVK_HIP_OK;
    // its hole (inclusive), clipped to that box: empty for a filled rectangle, a band as thick as the rectangle, or a hole outside the frame
    const long gx0 = std::max(x0 + b + 1, cx0), gy0 = std::max(y0 + b + 1, cy0), gx1 = std::min(x1 - a - 1, cx1), gy1 = std::min(y1 - a - 1, cy1);
    const bool hole = !fill && gx0 <= gx1 && gy0 <= gy1;
    const long w = cx1 - cx0 + 1, top = hole ? gy0 - cy0 : cy1 - cy0 + 1, bottom = hole ? cy1 - gy1 : 0, middle = hole ? gy1 - gy0 + 1 : 0;
    const long left = hole ? gx0 - cx0 : 0, side = hole ? left + (cx1 - gx1) : 0;
    const long full_px = (top + bottom) * w, total_px = full_px + middle * side;
    LVK_HIP_REQUIRE(ctx, total_px < (1L << 31));                                                           // the kernel indexes its pixels in 32 bits
    if (total_px == 0) return LVK_HIP_OK;
    const RectSpans s{(int)cx0, (int)cy0, (int)w, (int)top, (int)(gy1 + 1), (int)gy0, (int)left, (int)(gx1 + 1), (int)side, (uint32_t)full_px, (uint32_t)total_px};
    hipLaunchKernelGGL(k_draw_rect, dim3((unsigned)((total_px + 255) / 256)), dim3(256), 0, stream, (uint8_t*)d_dst, dst_step, s, pack3(colour));
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

constexpr int kMaxText = 256, kMaxTextScale = 32767, kMaxTextThickness = 65535;      // with these the kernel's coordinates stay in 32 bits

// cv::putText's place in the HUD, with the library's own font (tests/np_draw.py text_mask)
static int launch_draw_text(lvk_hip_ctx* ctx, hipStream_t stream, void* d_dst, int dst_step, int rows, int cols, const char* text, int x, int y,
                            const uint8_t colour[3], int scale, int thickness)
{
    LVK_HIP_REQUIRE(ctx, d_dst && rows > 0 && cols > 0 && dst_step >= 3 * cols && colour && text);
    LVK_HIP_REQUIRE(ctx, scale >= 1 && scale <= kMaxTextScale && thickness >= 1 && thickness <= kMaxTextThickness);
    const size_t n = strnlen(text, (size_t)kMaxText + 1);
    LVK_HIP_REQUIRE(ctx, n <= (size_t)kMaxText);
    if (n == 0) return LVK_HIP_OK;
    const long s = scale, g = (thickness - 1) / 2, top = (long)y - kGlyphH * s;                            // top row of the glyphs
    // the text's box (inclusive), clipped to the frame
    const long cx0 = std::max((long)x - g, 0L), cy0 = std::max(top - g, 0L);
    const long cx1 = std::min((long)x + ((long)kCellW * (long)n - 1) * s - 1 + g, (long)cols - 1), cy1 = std::min((long)y - 1 + g, (long)rows - 1);
    if (cx0 > cx1 || cy0 > cy1) return LVK_HIP_OK;
    const long w = cx1 - cx0 + 1, h = cy1 - cy0 + 1, u0 = cx0 - x, v0 = cy0 - top;
    LVK_HIP_REQUIRE(ctx, u0 + w + g < (1L << 31) && v0 + h + g < (1L << 31));                              // (a frame of more than 2^30 rows)
    void* d_text = nullptr;
    int rc = lvk_stage_params(ctx, stream, text, n, &d_text);
    if (rc != LVK_HIP_OK) return rc;
    hipLaunchKernelGGL(k_draw_text, dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)), dim3(64, 4), 0, stream, (const uint8_t*)d_text, (int)n,
                       (uint8_t*)d_dst, dst_step, (int)cx0, (int)cy0, (int)w, (int)h, (int)u0, (int)v0, scale, (int)g, pack3(colour));
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

extern "C" {

int lvk_hip_draw_grid(lvk_hip_ctx* ctx, void* d_dst, int dst_step, int rows, int cols, int grid_w, int grid_h, const uint8_t colour[3], int thickness)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_draw_grid(ctx, ctx->stream, d_dst, dst_step, rows, cols, grid_w, grid_h, colour, thickness);
}

int lvk_hip_draw_crosses(lvk_hip_ctx* ctx, void* d_dst, int dst_step, int rows, int cols, const float* pts_xy, int n,
                         float scale_x, float scale_y, const uint8_t colour[3], int cross_size, int thickness)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_draw_crosses(ctx, ctx->stream, d_dst, dst_step, rows, cols, pts_xy, n, scale_x, scale_y, colour, cross_size, thickness);
}

int lvk_hip_draw_points(lvk_hip_ctx* ctx, void* d_dst, int dst_step, int rows, int cols, const float* pts_xy, int n, float scale_x, float scale_y,
                        const uint8_t colour[3], int point_size)
{
    LVK_HIP_ENTRY(ctx);
    return launch_draw_points(ctx, ctx->stream, d_dst, dst_step, rows, cols, pts_xy, n, scale_x, scale_y, colour, point_size);
}

int lvk_hip_draw_rect(lvk_hip_ctx* ctx, void* d_dst, int dst_step, int rows, int cols, const int rect_xywh[4], const uint8_t colour[3], int thickness)
{
    LVK_HIP_ENTRY(ctx);
    return launch_draw_rect(ctx, ctx->stream, d_dst, dst_step, rows, cols, rect_xywh, colour, thickness);
}

int lvk_hip_draw_text(lvk_hip_ctx* ctx, void* d_dst, int dst_step, int rows, int cols, const char* text, int x, int y, const uint8_t colour[3],
                      int scale, int thickness)
{
    LVK_HIP_ENTRY(ctx);
    return launch_draw_text(ctx, ctx->stream, d_dst, dst_step, rows, cols, text, x, y, colour, scale, thickness);
}

int lvk_hip_text_size(const char* text, int scale, int thickness, int wh[2], int* baseline)
{
    if (!text || !wh || !baseline || scale < 1 || scale > kMaxTextScale || thickness < 1 || thickness > kMaxTextThickness) return LVK_HIP_ERR_ARG;
    const size_t n = strnlen(text, (size_t)kMaxText + 1);
    if (n > (size_t)kMaxText) return LVK_HIP_ERR_ARG;
    const int g = (thickness - 1) / 2;
    wh[0] = n ? (kCellW * (int)n - 1) * scale + 2 * g : 0;               // n cells less the last one's blank column
    wh[1] = kGlyphH * scale + 2 * g;
    *baseline = scale + g;                                                // the cell's blank row below the glyphs
    return LVK_HIP_OK;
}

} // extern "C"
