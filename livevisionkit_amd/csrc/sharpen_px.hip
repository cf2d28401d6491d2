// FSR robust contrast adaptive sharpening (RCAS) of ONE-channel (8UC1, VideoFrame::GRAY) and FOUR-channel (8UC4, VideoFrame::BGRA / RGBA) frames for
// gfx950: the kernels behind lvk_hip_sharpen_gray / _c4, the second half of ScalingFilter::filter on the frames the GRAY and four-channel stabilizer
// pushes emit.
//
// The reference's lvk::sharpen asserts CV_8UC3 (Functions/Image.cpp:208), so there is no one- or four-channel program to copy: both are DEFINED from the
// three-channel `rcas` program (FSR.cl:460-535) and run its per-pixel arithmetic under the arithmetic contract at the head of sharpen.hip.
//   GRAY: any channel of the three-channel program on (g, g, g) -- the program with one channel: lobe = min(max(lobe_0, -0.1875), 0) * sharp.
//   Four channels (c0, c1, c2, a): bytes 0 .. 2 are the three-channel program on (c0, c1, c2); byte 3 is the SOURCE pixel's alpha, copied.  The limiter
//     is built from the colour channels and bounds only them: a lobe applied to alpha could leave [0, 1] and wrap in the truncating conversion, and alpha
//     cannot join the limiter, whose three lobes are coupled through their maximum, without changing the colours.
// Out of place; border pixels (x or y on the frame edge) are copied, alpha included.
//
// Shape: that of k_rcas (sharpen.hip).  A thread owns 4 x RCAS_ROWS output pixels, loads the RCAS_ROWS + 2 source rows it needs at once and walks them
// with a rolling three-row window in registers; the limiter reciprocals come from the same two LDS tables, filled by the same expressions.  A pixel trait
// carries the load / store side:
//   GRAY: a thread's four pixels of a row are one (unaligned) dword load plus the byte on either side, and one dword store;
//   four channels: a 16-byte load plus the dword on either side, and one 16-byte store.
// The groups of a thread row are shifted left by the misalignment of its first destination row (0 .. 3 pixels, as in remap_one_strip_px), so that with a
// pitch that keeps the rows aligned alike every store is aligned whatever the base address is; a GRAY row that is not dword-aligned (odd pitches) leaves
// as bytes.  The first and the last group of a row, where the frame ends inside the group, go pixel by pixel.  No load touches a byte outside the
// cols * BPP bytes of a frame row (the side loads fall back to in-row addresses at the frame edge: what they return there belongs to border pixels), and
// only cols * BPP bytes of a destination row are written.
#include "lvk_hip_internal.hpp"

#include <cmath>

namespace {

constexpr int RCAS_PXT = 4, RCAS_STRIP_W = 64 * RCAS_PXT, RCAS_ROWS = 4;

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ float min_(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ float max_(float a, float b) { return __builtin_fmaxf(a, b); }

template <int N> struct PxN { float c[N]; };

// limiter reciprocals of the 256 possible ring extrema (FSR.cl:513-518, "these need to be high precision RCPs"), computed as k_rcas computes them so that the
// bytes match; one entry per thread of a 256-thread block, the caller puts the barrier behind it
__device__ __forceinline__ void rcas_fill_tables(float* __restrict__ s_rmin, float* __restrict__ s_rmax)
{
    const float v = (float)threadIdx.x * 0.00392156862f;
    // What the reference's kernel computes when it is compiled for this device: LLVM folds `-hitMin` into
    // min * (-1.0f / (4 mx4)), a correctly rounded divide; the hitMax reciprocal stays the device's v_rcp_f32.
    s_rmin[threadIdx.x] = 1.0f / (4.0f * v);                                   // native_recip(4 * mx4), negation folded in
    s_rmax[threadIdx.x] = __builtin_amdgcn_rcpf(fma_(4.0f, v, -4.0f));         // native_recip(4 * mn4 + peakC.y)
}

// FSR.cl:486-534 for one pixel of N colour channels, rcas_pixel of sharpen.hip with the channel count as a parameter (the same expressions in the same
// order, so that the bytes match): b above, h below, d left, f right, e centre.  Returns channel c in byte c, the bytes above N zero.
template <int N>
__device__ __forceinline__ uint32_t rcas_pixel(const PxN<N>& b, const PxN<N>& d, const PxN<N>& e, const PxN<N>& f, const PxN<N>& h, float sharp,
                                               const float* __restrict__ s_rmin, const float* __restrict__ s_rmax)
{
    float lobe_c[N];
#pragma unroll
    for (int c = 0; c < N; c++)                              // FSR.cl:503-521
    {
        const float mn4 = min_(b.c[c], min_(d.c[c], min_(f.c[c], h.c[c])));
        const float mx4 = max_(b.c[c], max_(d.c[c], max_(f.c[c], h.c[c])));
        // Byte offset 4 k of an extremum k * norm_factor in the tables, without a conversion or a left shift (both half-rate VALU
        // classes on gfx950, scripts/valu_peak.hip): 1020 (k norm) + 2 = 4 k + 2 - 8e-9 k, and adding 2^23 leaves that integer,
        // rounded to 4 k + 2 for every k in 0..255, in the low mantissa bits.
        const uint32_t omx = __float_as_uint(fma_(mx4, 1020.0f, 8388610.0f)) & 0x3fcu;
        const uint32_t omn = __float_as_uint(fma_(mn4, 1020.0f, 8388610.0f)) & 0x3fcu;
        const float hitMin = min_(mn4, e.c[c]) * *reinterpret_cast<const float*>(reinterpret_cast<const char*>(s_rmin) + omx);
        const float hitMax = (1.0f - max_(mx4, e.c[c])) * *reinterpret_cast<const float*>(reinterpret_cast<const char*>(s_rmax) + omn);
        lobe_c[c] = max_(-hitMin, hitMax);
    }
    float lobe_max = lobe_c[0];                              // max(lobe.z, max(lobe.y, lobe.x)); a NaN limiter loses
#pragma unroll
    for (int c = 1; c < N; c++) lobe_max = max_(lobe_c[c], lobe_max);
    const float lobe = min_(max_(lobe_max, -0.1875f), 0.0f) * sharp;   // FSR.cl:525
    const float a = fma_(4.0f, lobe, 1.0f);                  // FSR.cl:528, APrxMedRcpF1 (FSR.cl:70)
    const float rb = __uint_as_float(0x7ef19fffu - __float_as_uint(a));
    const float rcpL = rb * fma_(-rb, a, 2.0f);
    uint32_t px = 0;
#pragma unroll
    for (int c = 0; c < N; c++)                              // FSR.cl:529-531
    {
        const float v = fma_(((b.c[c] + d.c[c]) + h.c[c]) + f.c[c], lobe, e.c[c]) * rcpL;
        px |= ((uint32_t)(int)(v * 255.0f) & 0xffu) << (8 * c);
    }
    return px;
}

struct __attribute__((packed, aligned(1))) GrayWord { uint32_t w; };          // four GRAY pixels at any address
struct __attribute__((packed, aligned(4))) C4Quad { uint32_t w[4]; };         // four dword pixels at a multiple of 4

__device__ __forceinline__ float unorm(uint32_t byte) { return (float)byte * 0.00392156862f; }               // FSR.cl:484

struct GrayRcas
{
    static constexpr int BPP = 1, NC = 1;
    using Px = PxN<1>;
    static bool plane_ok(const void*, int) { return true; }                                                  // any base, any pitch
    static __device__ __forceinline__ uint32_t load_px(const uint8_t* p) { return *p; }
    static __device__ __forceinline__ Px unpack(uint32_t raw) { return Px{{unorm(raw & 0xffu)}}; }
    static __device__ __forceinline__ uint32_t keep(uint32_t sharpened, uint32_t /*centre*/) { return sharpened; }
    static __device__ __forceinline__ void store_px(uint8_t* p, uint32_t v) { *p = (uint8_t)v; }
    // one source row as a thread sees it: its four pixels, the pixel left of them and the pixel right of them
    struct Raw { uint32_t w, l, r; };
    static __device__ __forceinline__ Raw load_row(const uint8_t* rp, bool has_left, bool has_right)
    {
        return Raw{reinterpret_cast<const GrayWord*>(rp)->w, *(has_left ? rp - 1 : rp), *(has_right ? rp + 4 : rp + 3)};
    }
    static __device__ __forceinline__ uint32_t raw_px(const Raw& r, int k) { return k == 0 ? r.l : k == 5 ? r.r : (r.w >> (8 * (k - 1))) & 0xffu; }
    static __device__ __forceinline__ void store_group(uint8_t* p, const uint32_t out[RCAS_PXT])
    {
        if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) *reinterpret_cast<uint32_t*>(p) = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
        else
            for (int k = 0; k < RCAS_PXT; k++) p[k] = (uint8_t)out[k];
    }
};

struct C4Rcas
{
    static constexpr int BPP = 4, NC = 3;
    using Px = PxN<3>;
    static bool plane_ok(const void* p, int step) { return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)step) & 3u) == 0; }    // C4Pix::plane_ok's rule
    static __device__ __forceinline__ uint32_t load_px(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
    static __device__ __forceinline__ Px unpack(uint32_t raw) { return Px{{unorm(raw & 0xffu), unorm((raw >> 8) & 0xffu), unorm((raw >> 16) & 0xffu)}}; }
    static __device__ __forceinline__ uint32_t keep(uint32_t sharpened, uint32_t centre) { return sharpened | (centre & 0xff000000u); }   // the source's alpha
    static __device__ __forceinline__ void store_px(uint8_t* p, uint32_t v) { *reinterpret_cast<uint32_t*>(p) = v; }
    struct Raw { uint32_t w[RCAS_PXT], l, r; };
    static __device__ __forceinline__ Raw load_row(const uint8_t* rp, bool has_left, bool has_right)
    {
        const C4Quad q = *reinterpret_cast<const C4Quad*>(rp);
        return Raw{{q.w[0], q.w[1], q.w[2], q.w[3]}, load_px(has_left ? rp - 4 : rp), load_px(has_right ? rp + 16 : rp + 12)};
    }
    static __device__ __forceinline__ uint32_t raw_px(const Raw& r, int k) { return k == 0 ? r.l : k == 5 ? r.r : r.w[k - 1]; }
    static __device__ __forceinline__ void store_group(uint8_t* p, const uint32_t out[RCAS_PXT])
    {
        *reinterpret_cast<C4Quad*>(p) = C4Quad{{out[0], out[1], out[2], out[3]}};
    }
};

template <class Pix> struct RowOf { typename Pix::Px p[RCAS_PXT + 2]; };

template <class Pix>
__device__ __forceinline__ RowOf<Pix> unpack_row(const typename Pix::Raw& r)
{
    RowOf<Pix> o;
#pragma unroll
    for (int k = 0; k < RCAS_PXT + 2; k++) o.p[k] = Pix::unpack(Pix::raw_px(r, k));
    return o;
}

template <class Pix, int ROWS>
__global__ __launch_bounds__(256)
void k_rcas_px(const uint8_t* __restrict__ src, int src_step, int rows, int cols, uint8_t* __restrict__ dst, int dst_step, float sharp)
{
    constexpr int BPP = Pix::BPP;
    __shared__ float s_rmin[256], s_rmax[256];
    rcas_fill_tables(s_rmin, s_rmax);
    __syncthreads();

    const int y0 = ((int)blockIdx.y * 4 + (int)(threadIdx.x >> 6)) * ROWS;
    if (y0 >= rows) return;
    // pixels by which the thread row's first destination row lies past a boundary of RCAS_PXT pixels (wave-uniform; a row start is a multiple of BPP)
    const int mis = (int)((reinterpret_cast<uintptr_t>(dst + (long)y0 * dst_step) / BPP) & 3u);
    const int x0 = (int)blockIdx.x * RCAS_STRIP_W + (int)(threadIdx.x & 63) * RCAS_PXT - mis;
    if (x0 >= cols) return;                                          // (x0 + RCAS_PXT > 0 always: mis <= 3)

    if (x0 < 0 || x0 + RCAS_PXT > cols)                              // the frame ends inside the group: one pixel at a time
    {
        for (int y = y0; y < min(y0 + ROWS, rows); y++)
            for (int x = max(x0, 0); x < min(x0 + RCAS_PXT, cols); x++)
            {
                const uint8_t* pe = src + (long)y * src_step + BPP * (long)x;
                uint32_t px = Pix::load_px(pe);
                if (!(x == 0 || x >= cols - 1 || y == 0 || y >= rows - 1))
                    px = Pix::keep(rcas_pixel<Pix::NC>(Pix::unpack(Pix::load_px(pe - src_step)), Pix::unpack(Pix::load_px(pe - BPP)), Pix::unpack(px),
                                                       Pix::unpack(Pix::load_px(pe + BPP)), Pix::unpack(Pix::load_px(pe + src_step)), sharp, s_rmin, s_rmax), px);
                Pix::store_px(dst + (long)y * dst_step + BPP * (long)x, px);
            }
        return;
    }

    // Unconditional loads (no branches, so that all rows of a thread are in flight together): the row index is clamped into the image -- whatever a
    // clamped row returns belongs to border pixels, which are copied.  0 <= x0 and x0 + RCAS_PXT <= cols here.
    typename Pix::Raw raw[ROWS + 2];                                 // rows y0 - 1 .. y0 + ROWS
#pragma unroll
    for (int r = 0; r < ROWS + 2; r++)
        raw[r] = Pix::load_row(src + (long)min(max(y0 - 1 + r, 0), rows - 1) * src_step + BPP * (long)x0, x0 > 0, x0 + RCAS_PXT < cols);
    RowOf<Pix> win[3];
    win[0] = unpack_row<Pix>(raw[0]);
    win[1] = unpack_row<Pix>(raw[1]);
#pragma unroll
    for (int r = 0; r < ROWS; r++)
    {
        const int y = y0 + r;
        if (y >= rows) break;
        const RowOf<Pix>& up = win[r % 3];
        const RowOf<Pix>& mid = win[(r + 1) % 3];
        RowOf<Pix>& down = win[(r + 2) % 3];
        down = unpack_row<Pix>(raw[r + 2]);
        const bool border_row = y == 0 || y >= rows - 1;
        uint32_t out[RCAS_PXT];
#pragma unroll
        for (int p = 0; p < RCAS_PXT; p++)
        {
            const int x = x0 + p;
            const bool border = border_row || x == 0 || x >= cols - 1;              // FSR.cl:475-481: copied
            const uint32_t centre = Pix::raw_px(raw[r + 1], p + 1);
            const uint32_t px = rcas_pixel<Pix::NC>(up.p[p + 1], mid.p[p], mid.p[p + 1], mid.p[p + 2], down.p[p + 1], sharp, s_rmin, s_rmax);
            out[p] = border ? centre : Pix::keep(px, centre);
        }
        Pix::store_group(dst + (long)y * dst_step + BPP * (long)x0, out);
    }
}

// lvk::sharpen on a one- or four-channel frame
template <class Pix>
int launch_sharpen_px(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step, float sharpness)
{
    constexpr int BPP = Pix::BPP;
    LVK_HIP_REQUIRE(ctx, d_src != nullptr && d_dst != nullptr);
    LVK_HIP_REQUIRE(ctx, cols > 0 && rows > 0);
    LVK_HIP_REQUIRE(ctx, sharpness >= 0.0f && sharpness <= 1.0f);                // LVK_ASSERT_01, Image.cpp:210 (a NaN fails both)
    LVK_HIP_REQUIRE(ctx, src_step >= (long long)BPP * cols && dst_step >= (long long)BPP * cols);
    LVK_HIP_REQUIRE(ctx, Pix::plane_ok(d_src, src_step) && Pix::plane_ok(d_dst, dst_step));
    // the kernel reads the neighbours of what another thread writes
    LVK_HIP_REQUIRE(ctx, !lvk_pitched_overlap(d_src, src_step, rows, (long long)BPP * cols, d_dst, dst_step, rows, (long long)BPP * cols));
    const float sharp = exp2f(-2.0f * (1.0f - sharpness));                       // Image.cpp:227
    // (cols + 3: the 0 .. 3 pixels a misaligned destination row shifts its groups by)
    const dim3 block(256), grid((unsigned)((cols + 3 + RCAS_STRIP_W - 1) / RCAS_STRIP_W), (unsigned)((rows + 4 * RCAS_ROWS - 1) / (4 * RCAS_ROWS)));
    hipLaunchKernelGGL((k_rcas_px<Pix, RCAS_ROWS>), grid, block, 0, ctx->stream, (const uint8_t*)d_src, src_step, rows, cols, (uint8_t*)d_dst, dst_step, sharp);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

} // namespace

extern "C" {

int lvk_hip_sharpen_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step, float sharpness)
{
    LVK_HIP_ENTRY(ctx);
    return launch_sharpen_px<GrayRcas>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, sharpness);
}

int lvk_hip_sharpen_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step, float sharpness)
{
    LVK_HIP_ENTRY(ctx);
    return launch_sharpen_px<C4Rcas>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, sharpness);
}

} // extern "C"
