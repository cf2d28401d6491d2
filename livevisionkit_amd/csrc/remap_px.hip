// Dense remap of ONE-channel (8UC1, VideoFrame::GRAY) and FOUR-channel (8UC4, VideoFrame::BGRA / RGBA; BGRX is a BGRA frame) frames for gfx950: the kernels
// and launchers behind lvk_hip_remap_*_gray / _c4, lvk_hip_warpmesh_apply*_gray / _c4, lvk_hip_upscale_gray / _c4 and the stabilizer's GRAY and
// four-channel pushes.
//
// The reference's lvk::remap asserts CV_8UC3 (Functions/Image.cpp:32), so there is no one- or four-channel program to copy: each family is DEFINED from the
// three-channel non-YUV EASU program (above its pixel trait below; DESIGN.md sections 19 and 21) and runs easu_core (remap_core.hpp, the three-channel core,
// untouched).  Coordinate generators, the mesh in LDS, the XCD-aware strip order and the persistent grid of the overlap mode are the shared ones.
//
// One strip body, one set of kernels and one set of launchers serve both families; a pixel trait (GrayPix, C4Pix) carries what differs, the load / store
// side.  In both a thread's four adjacent output pixels are ONE aligned store: the strip is shifted left by the misalignment of the destination row (0 .. 3
// pixels), so that the store of every thread is aligned whatever the pitch and the base address are; only the first and the last group of a row, where the
// frame ends inside the group, leave pixel by pixel.
#include "remap_core.hpp"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- GRAY ---------------------------------------------------------------------------------------------------------------------------------------------
// Definition: the reference's non-YUV EASU program (FSR.cl:229-241 without YUV_INPUT) reads the luma of the edge analysis as
// channel 0 of the pixel; the twelve tap weights then depend on channel 0 alone, and every channel is accumulated, normalised, clamped to its own min / max
// of the four centre taps and converted on its own.  The remap of a one-channel frame g is channel 0 of that program run on the three-channel frame
// (g, c, c), for any constant c, background (bg, *, *).
//
// The kernels ARE that program: every tap is handed to easu_core as the pixel (v, 0, 0) with luma v, and the low byte of its result is kept.  easu_core is
// inlined here, so the two dead channels -- two thirds of the accumulate / normalise / clamp / convert work -- are removed by the compiler; the analysis and
// the weights are the same instructions in the same order.
//
// Load / store side, one byte per pixel:
//   * taps: the 4 x 4 byte window of a pixel is FOUR unaligned dword loads (rows sy - 1 .. sy + 2, columns sx - 1 .. sx + 2; the corner bytes are loaded
//     and not used), against four block-uniform row bases and one 32-bit offset per pixel, instead of 8 + 16 + 16 + 8 bytes;
//   * stores: a thread's four pixels are ONE dword, ragged groups leave as bytes.  A 64-lane wave writes 256 contiguous bytes of one row.
struct GrayPix
{
    static constexpr int BPP = 1;
    using Bg = uint8_t;                                              // the background as the launchers take it: the byte
    static bool bg_ok(Bg) { return true; }
    static uint32_t pack_bg(Bg bg) { return bg; }
    static bool plane_ok(const void* p, int step, int rows, int cols) { return remap_plane_ok(p, step, rows, cols, 1); }

    // the four rows of a pixel's tap window, each one column to the left of the pixel: block-uniform (scalar registers)
    static __device__ __forceinline__ TapBases bases(const uint8_t* __restrict__ src, int step)
    {
        return TapBases{src - 1, src + step - 1, src + 2 * (long)step - 1, src + 3 * (long)step - 1};
    }
    // one source pixel as easu_core consumes it: (v, 0, 0) with the luma of the non-YUV program, channel 0
    static __device__ __forceinline__ float4 make_tap(float byte_as_float)
    {
        const float v = byte_as_float * 0.00392156862f;                  // FSR.cl:205
        return make_float4(v, 0.0f, 0.0f, v);
    }
#define LVK_GRAY_BYTE(w, k) make_tap((float)(((w) >> (8 * (k))) & 0xffu))     /* v_cvt_f32_ubyte<k> */
    static __device__ __forceinline__ uint32_t gather(const TapBases& gb, int step, int sx, int sy, float ppx, float ppy)
    {
        // 1 <= sx <= cols - 5 and 1 <= sy <= rows - 5 here (interior pixels only): the window's columns sx - 1 .. sx + 2 and rows sy - 1 .. sy + 2 lie inside the
        // frame, so every byte of the four dwords is a byte of the frame (24-bit operands as in easu_gather)
        const uint32_t off = __umul24((uint32_t)(sy - 1), (uint32_t)step) + (uint32_t)sx;
        const uint32_t w0 = at_byte<U4B>(gb.r0, off).w;     // . b c .
        const uint32_t w1 = at_byte<U4B>(gb.r1, off).w;     // e f g h
        const uint32_t w2 = at_byte<U4B>(gb.r2, off).w;     // i j k l
        const uint32_t w3 = at_byte<U4B>(gb.r3, off).w;     // . n o .
        float4 t[12];
        t[TB] = LVK_GRAY_BYTE(w0, 1); t[TC] = LVK_GRAY_BYTE(w0, 2);
        t[TE] = LVK_GRAY_BYTE(w1, 0); t[TF] = LVK_GRAY_BYTE(w1, 1); t[TG] = LVK_GRAY_BYTE(w1, 2); t[TH_] = LVK_GRAY_BYTE(w1, 3);
        t[TI] = LVK_GRAY_BYTE(w2, 0); t[TJ] = LVK_GRAY_BYTE(w2, 1); t[TK] = LVK_GRAY_BYTE(w2, 2); t[TL] = LVK_GRAY_BYTE(w2, 3);
        t[TN] = LVK_GRAY_BYTE(w3, 1); t[TO] = LVK_GRAY_BYTE(w3, 2);
        return easu_core(t, ppx, ppy) & 0xffu;               // channel 0; the other two are dead code
    }
#undef LVK_GRAY_BYTE
    static __device__ __forceinline__ uint32_t border(const uint8_t* __restrict__ src, int step, int sx, int sy)
    {
        return src[__umul24((uint32_t)sy, (uint32_t)step) + (uint32_t)sx];
    }
    // a thread's group of PXT pixels, from column x0 of the row (drow + x0 is a multiple of 4): kept as the pair, the byte stores index the row
    struct Group { uint8_t* __restrict__ drow; int x0; };
    static __device__ __forceinline__ Group group(uint8_t* __restrict__ drow, int x0) { return Group{drow, x0}; }
    static __device__ __forceinline__ void store_group(const Group& g, const uint32_t px[PXT])
    {
        LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(g.drow + g.x0), px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24));
    }
    static __device__ __forceinline__ void store_ragged(const Group& g, int dst_cols, const uint32_t px[PXT])
    {
#pragma unroll
        for (int p = 0; p < PXT; p++)
            if (g.x0 + p >= 0 && g.x0 + p < dst_cols) g.drow[g.x0 + p] = (uint8_t)px[p];
    }
};

// ---- BGRA / RGBA ----------------------------------------------------------------------------------------------------------------------------------------
// Definition: in the reference's non-YUV EASU program (FSR.cl:229-241 without YUV_INPUT) the twelve tap weights depend on channel 0
// alone, and every channel is accumulated, normalised, clamped to its own min / max of the four centre taps and converted on its own: output channel k
// depends on input channels 0 and k only.  The remap of a four-channel frame (c0, c1, c2, a) is that program with a fourth channel accumulated under the
// same weights: bytes 0 .. 2 are the three-channel program on (c0, c1, c2), byte 3 is channel 1 of the three-channel program on (c0, a, a).
//
// The kernels ARE that program: easu_core is inlined TWICE on the same twelve taps, once with the pixel (c0, c1, c2) and once with (c0, a, 0), both with
// luma c0; bytes 0 .. 2 of the first result and byte 1 of the second are kept.  The analysis, the twelve weights, their sum and its reciprocal are the same
// expressions of the same values in both, so the compiler keeps one copy; what remains of the second call is one accumulate, normalise, clamp and convert
// (DESIGN.md section 21 has the instruction counts).
//
// Load / store side, one dword per pixel (both frames 4-byte aligned, both pitches multiples of 4: plane_ok refuses anything else):
//   * taps: a tap row is a dwordx2 (b c; n o) or a dwordx4 (e f g h; i j k l) against four block-uniform row bases and one 32-bit offset per pixel, as in
//     easu_gather; a tap is a whole dword of its row, so there is no byte_window shuffle and no 3-byte lane stride;
//   * stores: a thread's four pixels are ONE 16-byte store, ragged groups leave as dwords.  A 64-lane wave writes 1 KB of one row.
struct C4Pix
{
    static constexpr int BPP = 4;
    using Bg = const uint8_t*;                                       // the background as the launchers take it: four bytes
    static bool bg_ok(Bg bg) { return bg != nullptr; }
    static uint32_t pack_bg(Bg bg) { return (uint32_t)bg[0] | ((uint32_t)bg[1] << 8) | ((uint32_t)bg[2] << 16) | ((uint32_t)bg[3] << 24); }
    // a plane of dword pixels: well-formed, base and pitch multiples of 4
    static bool plane_ok(const void* p, int step, int rows, int cols)
    {
        return remap_plane_ok(p, step, rows, cols, 4) && ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)step) & 3u) == 0;
    }

    // the four rows of a pixel's tap window as easu_gather lays them out, in dword pixels: rows sy - 1 and sy + 2 from column sx, rows sy and sy + 1 from sx - 1
    static __device__ __forceinline__ TapBases bases(const uint8_t* __restrict__ src, int step)
    {
        return TapBases{src, src + step - 4, src + 2 * (long)step - 4, src + 3 * (long)step};
    }
    // one source pixel (a dword) as the two runs of easu_core consume it: COLOUR (c0, c1, c2), ALPHA (c0, a, 0); luma = channel 0 in both (FSR.cl:229-241)
    template <bool ALPHA>
    static __device__ __forceinline__ float4 make_tap(uint32_t w)
    {
        const float norm_factor = 0.00392156862f;               // FSR.cl:205
        const float c0 = (float)(w & 0xffu) * norm_factor;
        if (ALPHA) return make_float4(c0, (float)(w >> 24) * norm_factor, 0.0f, c0);
        return make_float4(c0, (float)((w >> 8) & 0xffu) * norm_factor, (float)((w >> 16) & 0xffu) * norm_factor, c0);
    }
    static __device__ __forceinline__ uint32_t gather(const TapBases& cb, int step, int sx, int sy, float ppx, float ppy)
    {
        // 1 <= sx <= cols - 5 and 1 <= sy <= rows - 5 here (interior pixels only): columns sx - 1 .. sx + 2 and rows sy - 1 .. sy + 2 lie inside the frame
        // (24-bit operands as in easu_gather)
        const uint32_t off = __umul24((uint32_t)(sy - 1), (uint32_t)step) + 4u * (uint32_t)sx;
        const U8B r0 = at_byte<U8B>(cb.r0, off);        // b, c
        const U16B r1 = at_byte<U16B>(cb.r1, off);      // e, f, g, h
        const U16B r2 = at_byte<U16B>(cb.r2, off);      // i, j, k, l
        const U8B r3 = at_byte<U8B>(cb.r3, off);        // n, o
        const uint32_t w[12] = { r0.w[0], r0.w[1], r1.w[0], r1.w[1], r1.w[2], r1.w[3], r2.w[0], r2.w[1], r2.w[2], r2.w[3], r3.w[0], r3.w[1] };   // TB .. TO
        float4 tc[12], ta[12];
#pragma unroll
        for (int k = 0; k < 12; k++) { tc[k] = make_tap<false>(w[k]); ta[k] = make_tap<true>(w[k]); }
        const uint32_t colour = easu_core(tc, ppx, ppy);           // 0x00 c2 c1 c0
        const uint32_t alpha = easu_core(ta, ppx, ppy);            // byte 1: a; its analysis and weights are the colour run's
        return colour | ((alpha & 0xff00u) << 16);
    }
    static __device__ __forceinline__ uint32_t border(const uint8_t* __restrict__ src, int step, int sx, int sy)
    {
        return at_byte<uint32_t>(src, __umul24((uint32_t)sy, (uint32_t)step) + 4u * (uint32_t)sx);
    }
    // a thread's group of PXT pixels, from column x0 of the row (a multiple of 16)
    struct Group { uint32_t* __restrict__ d; int x0; };
    static __device__ __forceinline__ Group group(uint8_t* __restrict__ drow, int x0) { return Group{reinterpret_cast<uint32_t*>(drow) + x0, x0}; }
    static __device__ __forceinline__ void store_group(const Group& g, const uint32_t px[PXT])
    {
        __builtin_nontemporal_store(u32x4{px[0], px[1], px[2], px[3]}, reinterpret_cast<u32x4*>(g.d));
    }
    static __device__ __forceinline__ void store_ragged(const Group& g, int dst_cols, const uint32_t px[PXT])
    {
#pragma unroll
        for (int p = 0; p < PXT; p++)
            if (g.x0 + p >= 0 && g.x0 + p < dst_cols) LVK_STREAM_STORE(g.d + p, px[p]);
    }
};

// ---- the strip body, the kernels and the launchers of both families ---------------------------------------------------------------------------------------
// columns a strip row can need: the frame's, plus the 0 .. 3 pixels a misaligned destination row is shifted by
__host__ __device__ __forceinline__ int px_span(int dst_cols) { return dst_cols + 3; }

template <class Pix, class Coord>
__device__ __forceinline__ void remap_one_strip_px(const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                                                   uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols, const Coord& coord, uint32_t bg,
                                                   int strip, int strips_x)
{
    const int sy_ = strip / strips_x, sx_ = strip - sy_ * strips_x;
    const int y = sy_ * STRIP_H + (int)(threadIdx.x >> 6);
    if (y >= dst_rows) return;                                        // (no barrier below: the mesh was staged before the strip walk)
    // (32-bit row offset against the block-uniform base, like the tap loads: a frame is < 4 GB)
    uint8_t* drow = dst + __umul24((uint32_t)y, (uint32_t)dst_step);
    const int mis = (int)((reinterpret_cast<uintptr_t>(drow) / Pix::BPP) & 3u);   // pixels past a boundary of PXT pixels (the row start is a multiple of BPP)
    const int x0 = sx_ * STRIP_W + (int)(threadIdx.x & 63) * PXT - mis;      // drow + BPP * x0 is a multiple of PXT * BPP
    if (x0 >= dst_cols || x0 + PXT <= 0) return;
    const TapBases tb = Pix::bases(src, src_step);
    uint32_t px[PXT];
#pragma unroll
    for (int p = 0; p < PXT; p++)
    {
        px[p] = 0;
        const int x = x0 + p;
        if (x >= 0 && x < dst_cols)
        {
            float subx, suby;
            coord(x, y, subx, suby);
            // shared tail of FSR.cl:380-402 / 429-451, as in remap_one_strip
            const int sx = (int)subx;
            const int sy = (int)suby;
            const float ppx = __builtin_amdgcn_fractf(subx);
            const float ppy = __builtin_amdgcn_fractf(suby);
            if (sx < 1 || sy < 1 || sx >= src_cols - 4 || sy >= src_rows - 4)
            {
                if (sx >= 0 && sx < src_cols && sy >= 0 && sy < src_rows) px[p] = Pix::border(src, src_step, sx, sy);
                else px[p] = bg;
            }
            else px[p] = Pix::gather(tb, src_step, sx, sy, ppx, ppy);
        }
    }
    const auto g = Pix::group(drow, x0);
    if (x0 >= 0 && x0 + PXT <= dst_cols) Pix::store_group(g, px);
    else Pix::store_ragged(g, dst_cols, px);
}

// the strip walk of remap_strip over px_span(dst_cols) columns
template <class Pix, class Coord>
__device__ __forceinline__ void remap_strip_px(const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                                               uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols, const Coord& coord, uint32_t bg)
{
    walk_strips(dst_rows, px_span(dst_cols), [&](int strip, int /*nstrips*/, int strips_x, int /*parity*/) __attribute__((always_inline)) {
        remap_one_strip_px<Pix>(src, src_step, src_rows, src_cols, dst, dst_step, dst_rows, dst_cols, coord, bg, strip, strips_x);
    });
}

// Pix: a profile tells the families apart by it.  CO: the same body under a name of its own for the persistent grid of the overlap mode (profiles tell the
// two apart).  remap.hip marks its `_co` kernels with LVK_CO_SCHEDULED, which is empty in the product build (the persistent grid, not an attribute, holds
// the occupancy down); a template cannot carry the marker on one instantiation only, so these kernels carry it on both forms: a definition that is ever
// given to it reaches the full-grid form as well.
template <class Pix, bool LENS, bool CO>
__global__ __launch_bounds__(256) LVK_REMAP_ATTR LVK_CO_SCHEDULED
void k_remap_homography_px(const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                           uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols,
                           int off_x, int off_y, HomographyArgs H, LensArgs L, uint32_t bg)
{
    with_homography_coord<LENS>(H, off_x, off_y, L, src_rows, src_cols, [&](const auto& coord) __attribute__((always_inline)) {
        remap_strip_px<Pix>(src, src_step, src_rows, src_cols, dst, dst_step, dst_rows, dst_cols, coord, bg);
    });
}

template <class Pix, bool LENS, bool CO>
__global__ __launch_bounds__(256) LVK_REMAP_ATTR LVK_CO_SCHEDULED
void k_remap_mesh_px(const uint8_t* __restrict__ src, int src_step, int rows, int cols, uint8_t* __restrict__ dst, int dst_step,
                     const float* __restrict__ mesh, int mesh_cols, int mesh_floats,
                     const LinTabEntry* __restrict__ xtab, const LinTabEntry* __restrict__ ytab, LensArgs L, uint32_t bg)
{
    LVK_WITH_MESH_COORD(LENS, L, rows, cols, remap_strip_px<Pix>(src, src_step, rows, cols, dst, dst_step, rows, cols, coord, bg))
}

template <class Pix>
__global__ __launch_bounds__(256) LVK_REMAP_ATTR
void k_remap_map_px(const uint8_t* __restrict__ src, int src_step, int rows, int cols, uint8_t* __restrict__ dst, int dst_step,
                    const uint8_t* __restrict__ map, int map_step, uint32_t bg)
{
    remap_strip_px<Pix>(src, src_step, rows, cols, dst, dst_step, rows, cols, MapCoord{map, map_step}, bg);
}

// lvk::upscale on a one- or four-channel frame (easu_scale, FSR.cl:324-358, defined for these frames as the remaps above are: DESIGN.md section 22): the same
// strip body under ScaleCoord; the source coordinate never leaves the image, so the border band is the nearest copy and the background is unreachable.
// Exact in every remap precision: it has no 1-LSB twin, like k_easu_scale.
template <class Pix>
__global__ __launch_bounds__(256) LVK_REMAP_ATTR
void k_easu_scale_px(const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                     uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols, float rsx, float rsy)
{
    remap_strip_px<Pix>(src, src_step, src_rows, src_cols, dst, dst_step, dst_rows, dst_cols, ScaleCoord{rsx, rsy}, 0u);
}

// The forms of family K for pixel PIX as launch_remap() takes them, [persistent grid][1-LSB][lens]: no twin, so both precisions are the one kernel (and a
// precision that is neither, which these launchers do not check, runs it too).  Here and not in remap_core.hpp: these kernels are plain templates on
// <Pix, LENS, CO>, not products of LVK_REMAP_KERNEL
#define LVK_PX_FORMS(K, PIX) RemapForms<decltype(&K<PIX, false, false>)>{ { { { K<PIX, false, false>, K<PIX, true, false> }, { K<PIX, false, false>, K<PIX, true, false> } }, \
                                                                            { { K<PIX, false, true>, K<PIX, true, true> }, { K<PIX, false, true>, K<PIX, true, true> } } } }

// the planes of a remap: both well-formed, and no byte shared -- the kernel reads a neighbourhood of what another thread writes
template <class Pix>
bool planes_ok(const void* src, int src_step, int src_rows, int src_cols, const void* dst, int dst_step, int dst_rows, int dst_cols)
{
    return Pix::plane_ok(src, src_step, src_rows, src_cols) && Pix::plane_ok(dst, dst_step, dst_rows, dst_cols) &&
           !lvk_pitched_overlap(src, src_step, src_rows, (long long)Pix::BPP * src_cols, dst, dst_step, dst_rows, (long long)Pix::BPP * dst_cols);
}

template <class Pix>
int launch_homography(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                      void* d_dst, int dst_step, int dst_rows, int dst_cols, int off_x, int off_y, const float H[9], typename Pix::Bg bg, const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, H != nullptr && Pix::bg_ok(bg) && planes_ok<Pix>(d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols));
    HomographyArgs args;
    std::memcpy(args.h, H, sizeof(args.h));
    launch_remap(ctx, LVK_PX_FORMS(k_remap_homography_px, Pix), o.lens != nullptr, dst_rows, px_span(dst_cols), o, 0, (const uint8_t*)d_src, src_step, src_rows, src_cols,
                 (uint8_t*)d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, args, o.lens ? *o.lens : LensArgs{}, Pix::pack_bg(bg));
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

template <class Pix>
int launch_mesh(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                const float* mesh, int mesh_rows, int mesh_cols, typename Pix::Bg bg, const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, Pix::bg_ok(bg) && remap_mesh_ok(mesh, mesh_rows, mesh_cols) && planes_ok<Pix>(d_src, src_step, rows, cols, d_dst, dst_step, rows, cols));
    return with_staged_mesh(ctx, o.stream, mesh, mesh_rows, mesh_cols, rows, cols, [&](const StagedMesh& m) {
        launch_remap(ctx, LVK_PX_FORMS(k_remap_mesh_px, Pix), o.lens != nullptr, rows, px_span(cols), o, 0, (const uint8_t*)d_src, src_step, rows, cols, (uint8_t*)d_dst, dst_step,
                     m.d_mesh, m.mesh_cols, m.mesh_floats, m.xtab, m.ytab, o.lens ? *o.lens : LensArgs{}, Pix::pack_bg(bg));
    });
}

template <class Pix>
int launch_map(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
               void* d_dst, int dst_step, const void* d_map, int map_step, typename Pix::Bg bg, const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, Pix::bg_ok(bg) && remap_map_ok(d_map, map_step, rows, cols) && planes_ok<Pix>(d_src, src_step, rows, cols, d_dst, dst_step, rows, cols));
    // (one kernel, no family to pick from: launched directly on the full grid; of `o` only the stream is read)
    hipLaunchKernelGGL(k_remap_map_px<Pix>, remap_grid(rows, px_span(cols)), dim3(256), 0, o.stream, (const uint8_t*)d_src, src_step, rows, cols, (uint8_t*)d_dst, dst_step,
                       (const uint8_t*)d_map, map_step, Pix::pack_bg(bg));
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// WarpMesh::apply on a one- or four-channel frame
template <class Pix>
int launch_warpmesh_apply_lens(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                               const float* mesh, int mesh_rows, int mesh_cols, typename Pix::Bg bg, const RemapLaunch& o)
{
    return route_warpmesh(ctx, mesh, mesh_rows, mesh_cols, rows, cols,
                          [&](const float H[9]) { return launch_homography<Pix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, rows, cols, 0, 0, H, bg, o); },
                          [&] { return launch_mesh<Pix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, o); });
}

// lvk::upscale(src, dst, size) on a one- or four-channel frame: the host side of lvk_launch_upscale (remap.hip)
template <class Pix>
int launch_upscale(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols, void* d_dst, int dst_step, int dst_rows, int dst_cols)
{
    LVK_HIP_REQUIRE(ctx, planes_ok<Pix>(d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols));
    LVK_HIP_REQUIRE(ctx, dst_cols >= src_cols && dst_rows >= src_rows);                         // Image.cpp:157
    if (dst_cols == src_cols && dst_rows == src_rows)                                           // Image.cpp:162-166
    {
        LVK_HIP_CHECK(ctx, hipMemcpy2DAsync(d_dst, (size_t)dst_step, d_src, (size_t)src_step, Pix::BPP * (size_t)src_cols, (size_t)src_rows,
                                            hipMemcpyDeviceToDevice, ctx->stream));
        return LVK_HIP_OK;
    }
    const float rsx = (float)src_cols / (float)dst_cols, rsy = (float)src_rows / (float)dst_rows;
    hipLaunchKernelGGL(k_easu_scale_px<Pix>, remap_grid(dst_rows, px_span(dst_cols)), dim3(256), 0, ctx->stream, (const uint8_t*)d_src, src_step, src_rows, src_cols,
                       (uint8_t*)d_dst, dst_step, dst_rows, dst_cols, rsx, rsy);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

} // namespace

// ---- the launchers the stabilizer calls (lvk_hip_internal.hpp) ------------------------------------------------------------------------------------------
int lvk_launch_remap_homography_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                                     void* d_dst, int dst_step, int dst_rows, int dst_cols, int off_x, int off_y, const float H[9], uint8_t bg, const RemapLaunch& o)
{
    return launch_homography<GrayPix>(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, H, bg, o);
}

int lvk_launch_remap_mesh_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                               const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg, const RemapLaunch& o)
{
    return launch_mesh<GrayPix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, o);
}

int lvk_launch_remap_map_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                              void* d_dst, int dst_step, const void* d_map, int map_step, uint8_t bg, const RemapLaunch& o)
{
    return launch_map<GrayPix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, d_map, map_step, bg, o);
}

int lvk_launch_warpmesh_apply_lens_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                        const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg, const RemapLaunch& o)
{
    return launch_warpmesh_apply_lens<GrayPix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, o);
}

int lvk_launch_remap_homography_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                                   void* d_dst, int dst_step, int dst_rows, int dst_cols, int off_x, int off_y, const float H[9], const uint8_t bg[4], const RemapLaunch& o)
{
    return launch_homography<C4Pix>(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, H, bg, o);
}

int lvk_launch_remap_mesh_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                             const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4], const RemapLaunch& o)
{
    return launch_mesh<C4Pix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, o);
}

int lvk_launch_remap_map_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                            void* d_dst, int dst_step, const void* d_map, int map_step, const uint8_t bg[4], const RemapLaunch& o)
{
    return launch_map<C4Pix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, d_map, map_step, bg, o);
}

int lvk_launch_warpmesh_apply_lens_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                      const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4], const RemapLaunch& o)
{
    return launch_warpmesh_apply_lens<C4Pix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, o);
}

extern "C" {

int lvk_hip_remap_homography_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                                  void* d_dst, int dst_step, int dst_rows, int dst_cols, int off_x, int off_y, const float H[9], uint8_t bg)
{
    LVK_HIP_ENTRY(ctx);
    return launch_homography<GrayPix>(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, H, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_remap_mesh_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols, void* d_dst, int dst_step,
                            const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg)
{
    LVK_HIP_ENTRY(ctx);
    return launch_mesh<GrayPix>(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_remap_map_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                           const void* d_map, int map_step, uint8_t bg)
{
    LVK_HIP_ENTRY(ctx);
    return launch_map<GrayPix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, d_map, map_step, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_warpmesh_apply_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg)
{
    LVK_HIP_ENTRY(ctx);
    return launch_warpmesh_apply_lens<GrayPix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_warpmesh_apply_lens_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                     const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg, const lvk_camera_params* lens)
{
    LVK_HIP_ENTRY(ctx);
    LVK_HIP_REQUIRE(ctx, lens != nullptr && rows > 1 && cols > 1);
    LensArgs a;
    const int rc = lens_args_of(ctx, lens, rows, cols, a);
    if (rc != LVK_HIP_OK) return rc;
    return launch_warpmesh_apply_lens<GrayPix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream, LVK_REMAP_EXACT, &a});
}

int lvk_hip_remap_homography_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                                void* d_dst, int dst_step, int dst_rows, int dst_cols, int off_x, int off_y, const float H[9], const uint8_t bg[4])
{
    LVK_HIP_ENTRY(ctx);
    return launch_homography<C4Pix>(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, H, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_remap_mesh_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols, void* d_dst, int dst_step,
                          const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4])
{
    LVK_HIP_ENTRY(ctx);
    return launch_mesh<C4Pix>(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_remap_map_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                         const void* d_map, int map_step, const uint8_t bg[4])
{
    LVK_HIP_ENTRY(ctx);
    return launch_map<C4Pix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, d_map, map_step, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_warpmesh_apply_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                              const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4])
{
    LVK_HIP_ENTRY(ctx);
    LVK_HIP_REQUIRE(ctx, bg != nullptr);
    return launch_warpmesh_apply_lens<C4Pix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_warpmesh_apply_lens_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                   const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4], const lvk_camera_params* lens)
{
    LVK_HIP_ENTRY(ctx);
    LVK_HIP_REQUIRE(ctx, bg != nullptr && lens != nullptr && rows > 1 && cols > 1);
    LensArgs a;
    const int rc = lens_args_of(ctx, lens, rows, cols, a);
    if (rc != LVK_HIP_OK) return rc;
    return launch_warpmesh_apply_lens<C4Pix>(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream, LVK_REMAP_EXACT, &a});
}

int lvk_hip_upscale_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols, void* d_dst, int dst_step, int dst_rows, int dst_cols)
{
    LVK_HIP_ENTRY(ctx);
    return launch_upscale<GrayPix>(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols);
}

int lvk_hip_upscale_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols, void* d_dst, int dst_step, int dst_rows, int dst_cols)
{
    LVK_HIP_ENTRY(ctx);
    return launch_upscale<C4Pix>(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols);
}

} // extern "C"
