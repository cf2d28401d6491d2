// Format conversion of packed 8-bit frames on the MI355X: VideoFrame::reformatTo (Data/VideoFrame.cpp:170-301) and ConversionFilter
// (Filters/ConversionFilter.cpp), i.e. OpenCV's CPU 8-bit cvtColor for BGR / BGRA / RGB / RGBA / YUV / GRAY.  Specification:
// tests/np_convert.py and DESIGN.md section 15.  Integer arithmetic only, so the output is bit-exact by construction.
//
// Two kernels per (source channels, destination channels, operation), on the context's stream:
//   k_convert_interior  when both row bases and both steps are multiples of 4: each lane converts a group of 16 pixels of one row, whose
//                       16 * C source and destination bytes are whole dwords, read and written as dwordx4.  Byte moves (shuffles, alpha,
//                       replication, channel extraction) are v_perm_b32 of the loaded dwords; the fixed-point maths is 24-bit
//                       multiply-adds on the extracted bytes.
//   k_convert_general   every other pixel: any pitch, any byte alignment, and the pixels of each row past its last whole group.  One
//                       pixel per lane, byte loads and stores.
// No byte outside the cols * C bytes of a destination row is written.  Same format on both sides: a 2-D copy.
#include "lvk_hip_internal.hpp"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int kGroup = 16;                 // pixels per lane on the interior path
constexpr int kBlock = 256;
constexpr long long kMaxBlocks = 2048;     // grid cap (memory-bound: stride the rest)

// operations; _B / _R name the channel order of the BGR-like side
enum Op
{
    OP_KEEP,        // 3/4 -> 3/4, same order (alpha 255 when added, dropped when removed)
    OP_SWAP,        // 3/4 -> 3/4, R and B exchanged (4 -> 4 keeps the alpha)
    OP_REP,         // GRAY -> 3/4: replicate, alpha 255
    OP_Y,           // YUV -> GRAY: channel 0
    OP_G2YUV,       // GRAY -> YUV: (g, 128, 128)
    OP_GRAY_B,      // BGR / BGRA -> GRAY
    OP_GRAY_R,      // RGB / RGBA -> GRAY
    OP_YUV_B,       // BGR / BGRA -> YUV
    OP_YUV_R,       // RGB / RGBA -> YUV
    OP_INV_B,       // YUV -> BGR / BGRA
    OP_INV_R,       // YUV -> RGB / RGBA
};

constexpr bool is_map(int op) { return op <= OP_G2YUV; }

// Byte map ops: where byte k of a destination group comes from.  >= 0: that source byte; -1: 0xff; -2: 0x80.
constexpr int byte_src(int op, int sc, int dc, int k)
{
    const int p = k / dc, c = k % dc;
    switch (op)
    {
    case OP_KEEP: return c == 3 ? -1 : p * sc + c;
    case OP_SWAP: return c == 3 ? (sc == 4 ? p * sc + 3 : -1) : p * sc + 2 - c;          // BGRA <-> RGBA keeps the alpha
    case OP_REP: return c == 3 ? -1 : p;
    case OP_Y: return p * 3;
    default: return c == 0 ? p : -2;                               // OP_G2YUV
    }
}

__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// RGB2Gray<uchar>, 15-bit
__device__ __forceinline__ int gray_of(int b, int g, int r) { return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15; }

// RGB2YCrCb_i<uchar> with the YUV coefficients, 14-bit; arithmetic shifts
__device__ __forceinline__ void yuv_of(int b, int g, int r, int& y, int& u, int& v)
{
    y = (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14;
    u = sat8(((b - y) * 8061 + (128 << 14) + 8192) >> 14);
    v = sat8(((r - y) * 14369 + (128 << 14) + 8192) >> 14);
}

// YCrCb2RGB_i<uchar> with the YUV coefficients
__device__ __forceinline__ void bgr_of(int y, int u, int v, int& b, int& g, int& r)
{
    const int du = u - 128, dv = v - 128;
    b = sat8(y + ((du * 33292 + 8192) >> 14));
    g = sat8(y + ((du * -6472 + dv * -9519 + 8192) >> 14));
    r = sat8(y + ((dv * 18678 + 8192) >> 14));
}

// One pixel of an arithmetic op: s[SC] source bytes -> d[DC] destination bytes
template <int SC, int DC, int OP>
__device__ __forceinline__ void convert_px(const int* s, int* d)
{
    if constexpr (OP == OP_GRAY_B || OP == OP_GRAY_R)
    {
        const int b = OP == OP_GRAY_B ? s[0] : s[2], r = OP == OP_GRAY_B ? s[2] : s[0];
        d[0] = gray_of(b, s[1], r);
    }
    else if constexpr (OP == OP_YUV_B || OP == OP_YUV_R)
    {
        const int b = OP == OP_YUV_B ? s[0] : s[2], r = OP == OP_YUV_B ? s[2] : s[0];
        yuv_of(b, s[1], r, d[0], d[1], d[2]);
    }
    else if constexpr (OP == OP_INV_B || OP == OP_INV_R)
    {
        int b, g, r;
        bgr_of(s[0], s[1], s[2], b, g, r);
        d[0] = OP == OP_INV_B ? b : r;
        d[1] = g;
        d[2] = OP == OP_INV_B ? r : b;
        if constexpr (DC == 4) d[3] = 255;
    }
    else
    {
#pragma unroll
        for (int k = 0; k < DC; k++)
        {
            const int from = byte_src(OP, SC, DC, k);
            d[k] = from >= 0 ? s[from] : from == -1 ? 255 : 128;
        }
    }
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));     // dword-aligned: global_load / store_dwordx4

__device__ __forceinline__ int byte_of(const uint32_t* w, int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu); }

// Destination dword j of a group of a byte map op: one v_perm_b32 when its four bytes come from two adjacent source dwords, two (OR-ed)
// when they straddle three; selector 0x0c gives 0x00, 0x0d gives 0xff, and the 0x80 bytes of OP_G2YUV are OR-ed in.
template <int SC, int DC, int OP>
__device__ __forceinline__ uint32_t map_dword(const uint32_t* w, int j)
{
    int lo = 1 << 20;
#pragma unroll
    for (int b = 0; b < 4; b++) { const int f = byte_src(OP, SC, DC, 4 * j + b); if (f >= 0) lo = std::min(lo, f >> 2); }
    uint32_t sel0 = 0, sel1 = 0, konst = 0;
    bool second = false;
#pragma unroll
    for (int b = 0; b < 4; b++)
    {
        const int f = byte_src(OP, SC, DC, 4 * j + b);
        uint32_t s0 = 0x0c, s1 = 0x0c;
        if (f == -1) s0 = 0x0d;
        else if (f == -2) konst |= 0x80u << (8 * b);
        else if ((f >> 2) - lo < 2) s0 = (uint32_t)(((f >> 2) - lo) * 4 + (f & 3));
        else { s1 = (uint32_t)(f & 3); second = true; }
        sel0 |= s0 << (8 * b);
        sel1 |= s1 << (8 * b);
    }
    if (lo == (1 << 20)) return konst | __builtin_amdgcn_perm(0u, 0u, sel0);
    const int hi = lo + 1 < 4 * SC ? lo + 1 : lo;
    uint32_t v = __builtin_amdgcn_perm(w[hi], w[lo], sel0);
    if (second) v |= __builtin_amdgcn_perm(0u, w[lo + 2 < 4 * SC ? lo + 2 : lo], sel1);
    return v | konst;
}

template <int SC, int DC, int OP>
__global__ __launch_bounds__(kBlock)
void k_convert_interior(const uint8_t* __restrict__ src, long long src_step, uint8_t* __restrict__ dst, long long dst_step, int rows,
                        int groups_per_row)
{
    const long long total = (long long)rows * groups_per_row;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < total; g += (long long)gridDim.x * kBlock)
    {
        const int y = (int)(g / groups_per_row), x = (int)(g - (long long)y * groups_per_row);
        const u32x4* sp = (const u32x4*)(src + y * src_step + (long long)x * (kGroup * SC));
        u32x4* dp = (u32x4*)(dst + y * dst_step + (long long)x * (kGroup * DC));
        uint32_t w[4 * SC], o[4 * DC];
#pragma unroll
        for (int i = 0; i < SC; i++)
        {
            const u32x4 v = sp[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
        if constexpr (is_map(OP))
        {
#pragma unroll
            for (int j = 0; j < 4 * DC; j++) o[j] = map_dword<SC, DC, OP>(w, j);
        }
        else
        {
#pragma unroll
            for (int j = 0; j < 4 * DC; j++) o[j] = 0;
#pragma unroll
            for (int p = 0; p < kGroup; p++)
            {
                int s[SC], d[DC];
#pragma unroll
                for (int c = 0; c < SC; c++) s[c] = byte_of(w, p * SC + c);
                convert_px<SC, DC, OP>(s, d);
#pragma unroll
                for (int c = 0; c < DC; c++) { const int k = p * DC + c; o[k >> 2] |= (uint32_t)d[c] << (8 * (k & 3)); }
            }
        }
#pragma unroll
        for (int i = 0; i < DC; i++) dp[i] = u32x4{o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]};
    }
}

// pixels x0 .. cols - 1 of every row, one per lane
template <int SC, int DC, int OP>
__global__ __launch_bounds__(kBlock)
void k_convert_general(const uint8_t* __restrict__ src, long long src_step, uint8_t* __restrict__ dst, long long dst_step, int rows, int x0,
                       int cols)
{
    const int width = cols - x0;
    const long long total = (long long)rows * width;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock)
    {
        const int y = (int)(i / width), x = x0 + (int)(i - (long long)y * width);
        const uint8_t* sp = src + y * src_step + (long long)x * SC;
        uint8_t* dp = dst + y * dst_step + (long long)x * DC;
        int s[SC], d[DC];
#pragma unroll
        for (int c = 0; c < SC; c++) s[c] = sp[c];
        convert_px<SC, DC, OP>(s, d);
#pragma unroll
        for (int c = 0; c < DC; c++) dp[c] = (uint8_t)d[c];
    }
}

unsigned blocks_for(long long work) { return (unsigned)std::min<long long>((work + kBlock - 1) / kBlock, kMaxBlocks); }

template <int SC, int DC, int OP>
hipError_t launch(hipStream_t stream, const uint8_t* src, long long src_step, uint8_t* dst, long long dst_step, int rows, int cols)
{
    const bool aligned = (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)src_step | (uintptr_t)dst_step) & 3) == 0;
    int x0 = 0;
    if (aligned && cols >= kGroup)
    {
        const int gpr = cols / kGroup;
        hipLaunchKernelGGL((k_convert_interior<SC, DC, OP>), dim3(blocks_for((long long)rows * gpr)), dim3(kBlock), 0, stream, src, src_step,
                           dst, dst_step, rows, gpr);
        x0 = gpr * kGroup;
    }
    if (x0 < cols)
        hipLaunchKernelGGL((k_convert_general<SC, DC, OP>), dim3(blocks_for((long long)rows * (cols - x0))), dim3(kBlock), 0, stream, src,
                           src_step, dst, dst_step, rows, x0, cols);
    return hipGetLastError();
}

// VideoFrame::reformatTo's dispatch (VideoFrame.cpp:186-301); src != dst
hipError_t dispatch(hipStream_t st, int from, int to, const uint8_t* s, long long ss, uint8_t* d, long long ds, int rows, int cols)
{
    enum { B = LVK_FORMAT_BGR, BA = LVK_FORMAT_BGRA, R = LVK_FORMAT_RGB, RA = LVK_FORMAT_RGBA, Y = LVK_FORMAT_YUV, G = LVK_FORMAT_GRAY };
#define LVK_CVT(F, T, SC, DC, OP) if (from == F && to == T) return launch<SC, DC, OP>(st, s, ss, d, ds, rows, cols)
    LVK_CVT(B, G, 3, 1, OP_GRAY_B);  LVK_CVT(B, R, 3, 3, OP_SWAP);  LVK_CVT(B, Y, 3, 3, OP_YUV_B);   LVK_CVT(B, RA, 3, 4, OP_SWAP);
    LVK_CVT(B, BA, 3, 4, OP_KEEP);
    LVK_CVT(BA, G, 4, 1, OP_GRAY_B); LVK_CVT(BA, R, 4, 3, OP_SWAP); LVK_CVT(BA, B, 4, 3, OP_KEEP);  LVK_CVT(BA, RA, 4, 4, OP_SWAP);
    LVK_CVT(BA, Y, 4, 3, OP_YUV_B);  // BGRA2BGR then BGR2YUV (:212-216): the alpha drops out either way
    LVK_CVT(R, G, 3, 1, OP_GRAY_R);  LVK_CVT(R, B, 3, 3, OP_SWAP);  LVK_CVT(R, Y, 3, 3, OP_YUV_R);   LVK_CVT(R, RA, 3, 4, OP_KEEP);
    LVK_CVT(R, BA, 3, 4, OP_SWAP);
    LVK_CVT(RA, G, 4, 1, OP_GRAY_R); LVK_CVT(RA, B, 4, 3, OP_SWAP); LVK_CVT(RA, R, 4, 3, OP_KEEP);  LVK_CVT(RA, BA, 4, 4, OP_SWAP);
    LVK_CVT(RA, Y, 4, 3, OP_YUV_R);
    LVK_CVT(Y, G, 3, 1, OP_Y);       LVK_CVT(Y, B, 3, 3, OP_INV_B); LVK_CVT(Y, BA, 3, 4, OP_INV_B); LVK_CVT(Y, R, 3, 3, OP_INV_R);
    LVK_CVT(Y, RA, 3, 4, OP_INV_R);  // dcn = 4: the destination receives YUV2RGB with alpha 255 (declared choice 1)
    LVK_CVT(G, R, 1, 3, OP_REP);     LVK_CVT(G, B, 1, 3, OP_REP);   LVK_CVT(G, RA, 1, 4, OP_REP);    LVK_CVT(G, BA, 1, 4, OP_REP);
    LVK_CVT(G, Y, 1, 3, OP_G2YUV);
#undef LVK_CVT
    return hipErrorInvalidValue;
}

} // namespace

extern "C" {

int lvk_hip_cvt_code_target(int code, int src_format, int dcn)
{
    enum { B = LVK_FORMAT_BGR, BA = LVK_FORMAT_BGRA, R = LVK_FORMAT_RGB, RA = LVK_FORMAT_RGBA, Y = LVK_FORMAT_YUV, G = LVK_FORMAT_GRAY };
    // code -> the destination of each accepted source format (-1: not accepted) in the order B, BA, R, RA, Y, G; and dcn of the code
    struct Row { int code, dcn, to[6]; };
    static const Row table[] = {
        {0, 4, {BA, -1, RA, -1, -1, -1}},       // BGR2BGRA = RGB2RGBA
        {1, 3, {-1, B, -1, R, -1, -1}},         // BGRA2BGR = RGBA2RGB
        {2, 4, {RA, -1, BA, -1, -1, -1}},       // BGR2RGBA = RGB2BGRA
        {3, 3, {-1, R, -1, B, -1, -1}},         // RGBA2BGR = BGRA2RGB
        {4, 3, {R, -1, B, -1, -1, -1}},         // BGR2RGB = RGB2BGR
        {5, 4, {-1, RA, -1, BA, -1, -1}},       // BGRA2RGBA = RGBA2BGRA
        {6, 1, {G, G, -1, -1, -1, -1}},         // BGR2GRAY (a BGRA frame too)
        {7, 1, {-1, -1, G, G, -1, -1}},         // RGB2GRAY (an RGBA frame too)
        {8, 3, {-1, -1, -1, -1, -1, B}},        // GRAY2BGR = GRAY2RGB
        {9, 4, {-1, -1, -1, -1, -1, BA}},       // GRAY2BGRA = GRAY2RGBA
        {10, 1, {G, G, -1, -1, -1, -1}},        // BGRA2GRAY (a BGR frame too)
        {11, 1, {-1, -1, G, G, -1, -1}},        // RGBA2GRAY (an RGB frame too)
        {82, 3, {Y, Y, -1, -1, -1, -1}},        // BGR2YUV (a BGRA frame too)
        {83, 3, {-1, -1, Y, Y, -1, -1}},        // RGB2YUV (an RGBA frame too)
        {84, 3, {-1, -1, -1, -1, B, -1}},       // YUV2BGR (dcn 4: BGRA)
        {85, 3, {-1, -1, -1, -1, R, -1}},       // YUV2RGB (dcn 4: RGBA)
    };
    if (src_format < 0 || src_format > G) return -1;
    for (const Row& row : table)
    {
        if (row.code != code) continue;
        const int to = row.to[src_format];
        if (to < 0) return -1;
        if ((code == 84 || code == 85) && dcn == 4) return code == 84 ? BA : RA;
        return dcn == 0 || dcn == row.dcn ? to : -1;
    }
    return -1;
}

int lvk_hip_reformat(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, int src_format, void* d_dst, int dst_step,
                     int dst_format)
{
    LVK_HIP_ENTRY(ctx);
    const int sc = lvk_format_channels(src_format), dc = lvk_format_channels(dst_format);
    if (!sc || !dc) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_reformat: unknown format (LVK_FORMAT_BGR .. LVK_FORMAT_GRAY)");
    LVK_HIP_REQUIRE(ctx, d_src && d_dst && rows > 0 && cols > 0);
    LVK_HIP_REQUIRE(ctx, (long long)src_step >= (long long)cols * sc && (long long)dst_step >= (long long)cols * dc);
    if (lvk_pitched_overlap(d_src, src_step, rows, (long long)cols * sc, d_dst, dst_step, rows, (long long)cols * dc)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_reformat: the source and destination overlap");
    if (src_format == dst_format)
    {
        LVK_HIP_CHECK(ctx, hipMemcpy2DAsync(d_dst, (size_t)dst_step, d_src, (size_t)src_step, (size_t)cols * sc, (size_t)rows,
                                            hipMemcpyDeviceToDevice, ctx->stream));
        return LVK_HIP_OK;
    }
    LVK_HIP_CHECK(ctx, dispatch(ctx->stream, src_format, dst_format, (const uint8_t*)d_src, src_step, (uint8_t*)d_dst, dst_step, rows, cols));
    return LVK_HIP_OK;
}

} // extern "C"
