// Dense remap of ONE-channel (8UC1, VideoFrame::GRAY) frames for gfx950: the kernels and launchers behind lvk_hip_remap_*_gray, lvk_hip_warpmesh_apply*_gray
// and the stabilizer's GRAY pushes.
//
// Definition: the reference's lvk::remap asserts CV_8UC3 (Functions/Image.cpp:32), so there is no one-channel program to copy.  Its
// non-YUV EASU program (FSR.cl:229-241 without YUV_INPUT) reads the luma of the edge analysis as channel 0 of the pixel; the twelve tap weights then depend on
// channel 0 alone, and every channel is accumulated, normalised, clamped to its own min / max of the four centre taps and converted on its own.  The remap of
// a one-channel frame g is channel 0 of that program run on the three-channel frame (g, c, c), for any constant c, background (bg, *, *).
//
// The kernels below ARE that program: every tap is handed to easu_core (remap_core.hpp, the three-channel core, untouched) as the pixel (v, 0, 0) with luma v,
// and the low byte of its result is kept.  easu_core is inlined here, so the two dead channels -- two thirds of the accumulate / normalise / clamp /
// convert work -- are removed by the compiler; the analysis and the weights are the same instructions in the same order.  Coordinate generators, the mesh in
// LDS, the XCD-aware strip order and the persistent grid of the overlap mode are the shared ones.
//
// What differs is the load / store side, for one byte per pixel:
//   * taps: the 4 x 4 byte window of a pixel is FOUR unaligned dword loads (rows sy - 1 .. sy + 2, columns sx - 1 .. sx + 2; the corner bytes are loaded
//     and not used), against four block-uniform row bases and one 32-bit offset per pixel, instead of 8 + 16 + 16 + 8 bytes;
//   * stores: a thread's four adjacent output pixels are ONE dword.  The strip is shifted left by the misalignment of the destination row (0 .. 3 bytes), so
//     that the dword of every thread is aligned whatever the pitch and the base address are; only the first and the last group of a row, where the frame
//     ends inside the dword, leave as bytes.  A 64-lane wave writes 256 contiguous bytes of one row.
#include "remap_core.hpp"

namespace {

// one source pixel as easu_core consumes it: (v, 0, 0) with the luma of the non-YUV program, channel 0
__device__ __forceinline__ float4 make_tap_gray(float byte_as_float)
{
    const float v = byte_as_float * 0.00392156862f;                  // FSR.cl:205
    return make_float4(v, 0.0f, 0.0f, v);
}
#define LVK_GRAY_BYTE(w, k) make_tap_gray((float)(((w) >> (8 * (k))) & 0xffu))     /* v_cvt_f32_ubyte<k> */

// the four rows of a pixel's tap window, each one column to the left of the pixel: block-uniform (scalar registers)
struct GrayBases { const uint8_t* __restrict__ r0; const uint8_t* __restrict__ r1; const uint8_t* __restrict__ r2; const uint8_t* __restrict__ r3; };
__device__ __forceinline__ GrayBases gray_bases(const uint8_t* __restrict__ src, int step)
{
    return GrayBases{src - 1, src + step - 1, src + 2 * (long)step - 1, src + 3 * (long)step - 1};
}

__device__ __forceinline__ uint32_t easu_gather_gray(const GrayBases& gb, int step, int sx, int sy, float ppx, float ppy)
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

// columns a strip row can need: the frame's, plus the 0 .. 3 a misaligned destination row is shifted by
__host__ __device__ __forceinline__ int gray_span(int dst_cols) { return dst_cols + 3; }

template <class Coord>
__device__ __forceinline__ void remap_one_strip_gray(const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                                                     uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols, const Coord& coord, uint32_t bg,
                                                     int strip, int strips_x)
{
    const int sy_ = strip / strips_x, sx_ = strip - sy_ * strips_x;
    const int y = sy_ * STRIP_H + (int)(threadIdx.x >> 6);
    if (y >= dst_rows) return;                                        // (no barrier below: the mesh was staged before the strip walk)
    // (32-bit row offset against the block-uniform base, like the tap loads: a frame is < 4 GB)
    uint8_t* drow = dst + __umul24((uint32_t)y, (uint32_t)dst_step);
    const int mis = (int)(reinterpret_cast<uintptr_t>(drow) & 3u);
    const int x0 = sx_ * STRIP_W + (int)(threadIdx.x & 63) * PXT - mis;      // drow + x0 is a multiple of 4
    if (x0 >= dst_cols || x0 + PXT <= 0) return;
    const GrayBases gb = gray_bases(src, src_step);
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
                if (sx >= 0 && sx < src_cols && sy >= 0 && sy < src_rows) px[p] = src[__umul24((uint32_t)sy, (uint32_t)src_step) + (uint32_t)sx];
                else px[p] = bg;
            }
            else px[p] = easu_gather_gray(gb, src_step, sx, sy, ppx, ppy);
        }
    }
    if (x0 >= 0 && x0 + PXT <= dst_cols)
        LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(drow + x0), px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24));
    else
#pragma unroll
        for (int p = 0; p < PXT; p++)
            if (x0 + p >= 0 && x0 + p < dst_cols) drow[x0 + p] = (uint8_t)px[p];
}

// the strip walk of remap_strip over gray_span(dst_cols) columns
template <class Coord>
__device__ __forceinline__ void remap_strip_gray(const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                                                 uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols, const Coord& coord, uint32_t bg)
{
    walk_strips(dst_rows, gray_span(dst_cols), [&](int strip, int /*nstrips*/, int strips_x, int /*parity*/) __attribute__((always_inline)) {
        remap_one_strip_gray(src, src_step, src_rows, src_cols, dst, dst_step, dst_rows, dst_cols, coord, bg, strip, strips_x);
    });
}

// CO: the same body under a name of its own for the persistent grid of the overlap mode (profiles tell the two apart).  remap.hip marks its `_co` kernels
// with LVK_CO_SCHEDULED, which is empty in the product build (the persistent grid, not an attribute, holds the occupancy down); a template cannot carry the
// marker on one instantiation only, so these kernels carry it on both forms: a definition that is ever given to it reaches the full-grid form as well.
template <bool LENS, bool CO>
__global__ __launch_bounds__(256) LVK_REMAP_ATTR LVK_CO_SCHEDULED
void k_remap_homography_gray(const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                             uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols,
                             int off_x, int off_y, HomographyArgs H, LensArgs L, uint32_t bg)
{
    with_homography_coord<LENS>(H, off_x, off_y, L, src_rows, src_cols, [&](const auto& coord) __attribute__((always_inline)) {
        remap_strip_gray(src, src_step, src_rows, src_cols, dst, dst_step, dst_rows, dst_cols, coord, bg);
    });
}

template <bool LENS, bool CO>
__global__ __launch_bounds__(256) LVK_REMAP_ATTR LVK_CO_SCHEDULED
void k_remap_mesh_gray(const uint8_t* __restrict__ src, int src_step, int rows, int cols, uint8_t* __restrict__ dst, int dst_step,
                       const float* __restrict__ mesh, int mesh_cols, int mesh_floats,
                       const LinTabEntry* __restrict__ xtab, const LinTabEntry* __restrict__ ytab, LensArgs L, uint32_t bg)
{
    LVK_WITH_MESH_COORD(LENS, L, rows, cols, remap_strip_gray(src, src_step, rows, cols, dst, dst_step, rows, cols, coord, bg))
}

__global__ __launch_bounds__(256) LVK_REMAP_ATTR
void k_remap_map_gray(const uint8_t* __restrict__ src, int src_step, int rows, int cols, uint8_t* __restrict__ dst, int dst_step,
                      const uint8_t* __restrict__ map, int map_step, uint32_t bg)
{
    remap_strip_gray(src, src_step, rows, cols, dst, dst_step, rows, cols, MapCoord{map, map_step}, bg);
}

// The forms of a one-channel family as launch_remap() takes them, [persistent grid][1-LSB][lens]: no twin, so both precisions are the one kernel (and a
// precision that is neither, which the one-channel launchers do not check, runs it too).  Here and not in remap_core.hpp: these kernels are plain
// templates on <LENS, CO>, not products of LVK_REMAP_KERNEL
#define LVK_GRAY_FORMS(K) RemapForms<decltype(&K<false, false>)>{ { { { K<false, false>, K<true, false> }, { K<false, false>, K<true, false> } }, \
                                                                    { { K<false, true>, K<true, true> }, { K<false, true>, K<true, true> } } } }

// the planes of a one-channel remap: both well-formed, and no byte shared -- the kernel reads a neighbourhood of what another thread writes
bool gray_planes_ok(const void* src, int src_step, int src_rows, int src_cols, const void* dst, int dst_step, int dst_rows, int dst_cols)
{
    return remap_plane_ok(src, src_step, src_rows, src_cols, 1) && remap_plane_ok(dst, dst_step, dst_rows, dst_cols, 1) &&
           !lvk_pitched_overlap(src, src_step, src_rows, src_cols, dst, dst_step, dst_rows, dst_cols);
}

} // namespace

int lvk_launch_remap_homography_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                                     void* d_dst, int dst_step, int dst_rows, int dst_cols, int off_x, int off_y, const float H[9], uint8_t bg, const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, H != nullptr && gray_planes_ok(d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols));
    HomographyArgs args;
    std::memcpy(args.h, H, sizeof(args.h));
    launch_remap(ctx, LVK_GRAY_FORMS(k_remap_homography_gray), o.lens != nullptr, dst_rows, gray_span(dst_cols), o, 0, (const uint8_t*)d_src, src_step, src_rows, src_cols,
                 (uint8_t*)d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, args, o.lens ? *o.lens : LensArgs{}, (uint32_t)bg);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

int lvk_launch_remap_mesh_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                               const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg, const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, remap_mesh_ok(mesh, mesh_rows, mesh_cols) && gray_planes_ok(d_src, src_step, rows, cols, d_dst, dst_step, rows, cols));
    return with_staged_mesh(ctx, o.stream, mesh, mesh_rows, mesh_cols, rows, cols, [&](const StagedMesh& m) {
        launch_remap(ctx, LVK_GRAY_FORMS(k_remap_mesh_gray), o.lens != nullptr, rows, gray_span(cols), o, 0, (const uint8_t*)d_src, src_step, rows, cols, (uint8_t*)d_dst, dst_step,
                     m.d_mesh, m.mesh_cols, m.mesh_floats, m.xtab, m.ytab, o.lens ? *o.lens : LensArgs{}, (uint32_t)bg);
    });
}

int lvk_launch_remap_map_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                              void* d_dst, int dst_step, const void* d_map, int map_step, uint8_t bg, const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, remap_plane_ok(d_map, map_step, rows, cols, 8) && gray_planes_ok(d_src, src_step, rows, cols, d_dst, dst_step, rows, cols));
    LVK_HIP_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_map) | (uintptr_t)map_step) & 7u) == 0);
    // (one kernel, no family to pick from: launched directly on the full grid; of `o` only the stream is read)
    hipLaunchKernelGGL(k_remap_map_gray, remap_grid(rows, gray_span(cols)), dim3(256), 0, o.stream, (const uint8_t*)d_src, src_step, rows, cols, (uint8_t*)d_dst, dst_step,
                       (const uint8_t*)d_map, map_step, (uint32_t)bg);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// WarpMesh::apply on a one-channel frame: a 2 x 2 mesh goes through the homography kernel, anything larger through the mesh kernel
int lvk_launch_warpmesh_apply_lens_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                        const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg, const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, remap_mesh_ok(mesh, mesh_rows, mesh_cols));
    if (mesh_rows == 2 && mesh_cols == 2)
    {
        float H[9];
        lvkh::mesh2x2_to_homography(mesh, rows, cols, H);
        return lvk_launch_remap_homography_gray(ctx, d_src, src_step, rows, cols, d_dst, dst_step, rows, cols, 0, 0, H, bg, o);
    }
    return lvk_launch_remap_mesh_gray(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, o);
}

extern "C" {

int lvk_hip_remap_homography_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                                  void* d_dst, int dst_step, int dst_rows, int dst_cols, int off_x, int off_y, const float H[9], uint8_t bg)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_remap_homography_gray(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, H, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_remap_mesh_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols, void* d_dst, int dst_step,
                            const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_remap_mesh_gray(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_remap_map_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                           const void* d_map, int map_step, uint8_t bg)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_remap_map_gray(ctx, d_src, src_step, rows, cols, d_dst, dst_step, d_map, map_step, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_warpmesh_apply_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_warpmesh_apply_lens_gray(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_warpmesh_apply_lens_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                     const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg, const lvk_camera_params* lens)
{
    LVK_HIP_ENTRY(ctx);
    LVK_HIP_REQUIRE(ctx, lens != nullptr && rows > 1 && cols > 1);
    LensModel m; LensArgs a;
    const int rc = lvk_lens_model_build(*lens, rows, cols, m);
    if (rc != LVK_HIP_OK) return ctx->fail(rc, "invalid camera profile");
    std::memcpy(a.f, m.f, sizeof(a.f));
    return lvk_launch_warpmesh_apply_lens_gray(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream, LVK_REMAP_EXACT, &a});
}

} // extern "C"
