// Dense remap of FOUR-channel (8UC4, VideoFrame::BGRA / RGBA; BGRX is a BGRA frame) frames for gfx950: the kernels and launchers behind lvk_hip_remap_*_c4,
// lvk_hip_warpmesh_apply*_c4 and the stabilizer's four-channel pushes.
//
// Definition: the reference's lvk::remap asserts CV_8UC3 (Functions/Image.cpp:32), so there is no four-channel program to copy.  In its
// non-YUV EASU program (FSR.cl:229-241 without YUV_INPUT) the twelve tap weights depend on channel 0 alone, and every channel is accumulated, normalised,
// clamped to its own min / max of the four centre taps and converted on its own: output channel k depends on input channels 0 and k only.  The remap of a
// four-channel frame (c0, c1, c2, a) is that program with a fourth channel accumulated under the same weights: bytes 0 .. 2 are the three-channel program on
// (c0, c1, c2), byte 3 is channel 1 of the three-channel program on (c0, a, a).
//
// The kernels below ARE that program: easu_core (remap_core.hpp, the three-channel core, untouched) is inlined TWICE on the same twelve taps, once with the
// pixel (c0, c1, c2) and once with (c0, a, 0), both with luma c0; bytes 0 .. 2 of the first result and byte 1 of the second are kept.  The analysis, the
// twelve weights, their sum and its reciprocal are the same expressions of the same values in both, so the compiler keeps one copy; what remains of the
// second call is one accumulate, normalise, clamp and convert (DESIGN.md section 21 has the instruction counts).  Coordinate generators, the mesh in LDS,
// the XCD-aware strip order and the persistent grid of the overlap mode are the shared ones.
//
// What differs is the load / store side, for one dword per pixel (both frames 4-byte aligned, both pitches multiples of 4: the launchers refuse anything else):
//   * taps: a tap row is a dwordx2 (b c; n o) or a dwordx4 (e f g h; i j k l) against four block-uniform row bases and one 32-bit offset per pixel, as in
//     easu_gather; a tap is a whole dword of its row, so there is no byte_window shuffle and no 3-byte lane stride;
//   * stores: a thread's four adjacent output pixels are ONE 16-byte store.  The strip is shifted left by the misalignment of the destination row (0 .. 3
//     pixels), so that the store of every thread is 16-byte aligned whatever multiple of 4 the row starts at; only the first and the last group of a row,
//     where the frame ends inside the 16 bytes, leave as dwords.  A 64-lane wave writes 1 KB of one row.
#include "remap_core.hpp"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the four rows of a pixel's tap window as easu_gather lays them out, in dword pixels: rows sy - 1 and sy + 2 from column sx, rows sy and sy + 1 from sx - 1
struct C4Bases { const uint8_t* __restrict__ r0; const uint8_t* __restrict__ r1; const uint8_t* __restrict__ r2; const uint8_t* __restrict__ r3; };
__device__ __forceinline__ C4Bases c4_bases(const uint8_t* __restrict__ src, int step)
{
    return C4Bases{src, src + step - 4, src + 2 * (long)step - 4, src + 3 * (long)step};
}

// one source pixel (a dword) as the two runs of easu_core consume it: COLOUR (c0, c1, c2), ALPHA (c0, a, 0); luma = channel 0 in both (FSR.cl:229-241)
template <bool ALPHA>
__device__ __forceinline__ float4 make_tap_c4(uint32_t w)
{
    const float norm_factor = 0.00392156862f;               // FSR.cl:205
    const float c0 = (float)(w & 0xffu) * norm_factor;
    if (ALPHA) return make_float4(c0, (float)(w >> 24) * norm_factor, 0.0f, c0);
    return make_float4(c0, (float)((w >> 8) & 0xffu) * norm_factor, (float)((w >> 16) & 0xffu) * norm_factor, c0);
}

__device__ __forceinline__ uint32_t easu_gather_c4(const C4Bases& cb, int step, int sx, int sy, float ppx, float ppy)
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
    for (int k = 0; k < 12; k++) { tc[k] = make_tap_c4<false>(w[k]); ta[k] = make_tap_c4<true>(w[k]); }
    const uint32_t colour = easu_core(tc, ppx, ppy);           // 0x00 c2 c1 c0
    const uint32_t alpha = easu_core(ta, ppx, ppy);            // byte 1: a; its analysis and weights are the colour run's
    return colour | ((alpha & 0xff00u) << 16);
}

// columns a strip row can need: the frame's, plus the 0 .. 3 pixels a destination row that does not start on 16 bytes is shifted by
__host__ __device__ __forceinline__ int c4_span(int dst_cols) { return dst_cols + 3; }

template <class Coord>
__device__ __forceinline__ void remap_one_strip_c4(const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                                                   uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols, const Coord& coord, uint32_t bg,
                                                   int strip, int strips_x)
{
    const int sy_ = strip / strips_x, sx_ = strip - sy_ * strips_x;
    const int y = sy_ * STRIP_H + (int)(threadIdx.x >> 6);
    if (y >= dst_rows) return;                                        // (no barrier below: the mesh was staged before the strip walk)
    // (32-bit row offset against the block-uniform base, like the tap loads: a frame is < 4 GB)
    uint8_t* drow = dst + __umul24((uint32_t)y, (uint32_t)dst_step);
    const int mis = (int)((reinterpret_cast<uintptr_t>(drow) >> 2) & 3u);   // pixels past a 16-byte boundary (the row start is a multiple of 4)
    const int x0 = sx_ * STRIP_W + (int)(threadIdx.x & 63) * PXT - mis;      // drow + 4 * x0 is a multiple of 16
    if (x0 >= dst_cols || x0 + PXT <= 0) return;
    const C4Bases cb = c4_bases(src, src_step);
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
                if (sx >= 0 && sx < src_cols && sy >= 0 && sy < src_rows) px[p] = at_byte<uint32_t>(src, __umul24((uint32_t)sy, (uint32_t)src_step) + 4u * (uint32_t)sx);
                else px[p] = bg;
            }
            else px[p] = easu_gather_c4(cb, src_step, sx, sy, ppx, ppy);
        }
    }
    uint32_t* d = reinterpret_cast<uint32_t*>(drow) + x0;
    if (x0 >= 0 && x0 + PXT <= dst_cols)
        __builtin_nontemporal_store(u32x4{px[0], px[1], px[2], px[3]}, reinterpret_cast<u32x4*>(d));
    else
#pragma unroll
        for (int p = 0; p < PXT; p++)
            if (x0 + p >= 0 && x0 + p < dst_cols) LVK_STREAM_STORE(d + p, px[p]);
}

// the strip walk of remap_strip over c4_span(dst_cols) columns
template <class Coord>
__device__ __forceinline__ void remap_strip_c4(const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                                               uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols, const Coord& coord, uint32_t bg)
{
    walk_strips(dst_rows, c4_span(dst_cols), [&](int strip, int /*nstrips*/, int strips_x, int /*parity*/) __attribute__((always_inline)) {
        remap_one_strip_c4(src, src_step, src_rows, src_cols, dst, dst_step, dst_rows, dst_cols, coord, bg, strip, strips_x);
    });
}

// CO: the same body under a name of its own for the persistent grid of the overlap mode, as in remap_gray.hip
template <bool LENS, bool CO>
__global__ __launch_bounds__(256) LVK_REMAP_ATTR LVK_CO_SCHEDULED
void k_remap_homography_c4(const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                           uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols,
                           int off_x, int off_y, HomographyArgs H, LensArgs L, uint32_t bg)
{
    with_homography_coord<LENS>(H, off_x, off_y, L, src_rows, src_cols, [&](const auto& coord) __attribute__((always_inline)) {
        remap_strip_c4(src, src_step, src_rows, src_cols, dst, dst_step, dst_rows, dst_cols, coord, bg);
    });
}

template <bool LENS, bool CO>
__global__ __launch_bounds__(256) LVK_REMAP_ATTR LVK_CO_SCHEDULED
void k_remap_mesh_c4(const uint8_t* __restrict__ src, int src_step, int rows, int cols, uint8_t* __restrict__ dst, int dst_step,
                     const float* __restrict__ mesh, int mesh_cols, int mesh_floats,
                     const LinTabEntry* __restrict__ xtab, const LinTabEntry* __restrict__ ytab, LensArgs L, uint32_t bg)
{
    LVK_WITH_MESH_COORD(LENS, L, rows, cols, remap_strip_c4(src, src_step, rows, cols, dst, dst_step, rows, cols, coord, bg))
}

__global__ __launch_bounds__(256) LVK_REMAP_ATTR
void k_remap_map_c4(const uint8_t* __restrict__ src, int src_step, int rows, int cols, uint8_t* __restrict__ dst, int dst_step,
                    const uint8_t* __restrict__ map, int map_step, uint32_t bg)
{
    remap_strip_c4(src, src_step, rows, cols, dst, dst_step, rows, cols, MapCoord{map, map_step}, bg);
}

// The forms of a four-channel family as launch_remap() takes them, [persistent grid][1-LSB][lens]: no twin, so both precisions are the one kernel
#define LVK_C4_FORMS(K) RemapForms<decltype(&K<false, false>)>{ { { { K<false, false>, K<true, false> }, { K<false, false>, K<true, false> } }, \
                                                                  { { K<false, true>, K<true, true> }, { K<false, true>, K<true, true> } } } }

// a plane of dword pixels: well-formed, base and pitch multiples of 4
bool c4_plane_ok(const void* p, int step, int rows, int cols)
{
    return remap_plane_ok(p, step, rows, cols, 4) && ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)step) & 3u) == 0;
}

// the planes of a four-channel remap: both well-formed, and no byte shared -- the kernel reads a neighbourhood of what another thread writes
bool c4_planes_ok(const void* src, int src_step, int src_rows, int src_cols, const void* dst, int dst_step, int dst_rows, int dst_cols)
{
    return c4_plane_ok(src, src_step, src_rows, src_cols) && c4_plane_ok(dst, dst_step, dst_rows, dst_cols) &&
           !lvk_pitched_overlap(src, src_step, src_rows, 4ll * src_cols, dst, dst_step, dst_rows, 4ll * dst_cols);
}

uint32_t pack_bg4(const uint8_t bg[4]) { return (uint32_t)bg[0] | ((uint32_t)bg[1] << 8) | ((uint32_t)bg[2] << 16) | ((uint32_t)bg[3] << 24); }

} // namespace

int lvk_launch_remap_homography_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                                   void* d_dst, int dst_step, int dst_rows, int dst_cols, int off_x, int off_y, const float H[9], const uint8_t bg[4], const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, H != nullptr && bg != nullptr && c4_planes_ok(d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols));
    HomographyArgs args;
    std::memcpy(args.h, H, sizeof(args.h));
    launch_remap(ctx, LVK_C4_FORMS(k_remap_homography_c4), o.lens != nullptr, dst_rows, c4_span(dst_cols), o, 0, (const uint8_t*)d_src, src_step, src_rows, src_cols,
                 (uint8_t*)d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, args, o.lens ? *o.lens : LensArgs{}, pack_bg4(bg));
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

int lvk_launch_remap_mesh_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                             const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4], const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, bg != nullptr && remap_mesh_ok(mesh, mesh_rows, mesh_cols) && c4_planes_ok(d_src, src_step, rows, cols, d_dst, dst_step, rows, cols));
    return with_staged_mesh(ctx, o.stream, mesh, mesh_rows, mesh_cols, rows, cols, [&](const StagedMesh& m) {
        launch_remap(ctx, LVK_C4_FORMS(k_remap_mesh_c4), o.lens != nullptr, rows, c4_span(cols), o, 0, (const uint8_t*)d_src, src_step, rows, cols, (uint8_t*)d_dst, dst_step,
                     m.d_mesh, m.mesh_cols, m.mesh_floats, m.xtab, m.ytab, o.lens ? *o.lens : LensArgs{}, pack_bg4(bg));
    });
}

int lvk_launch_remap_map_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                            void* d_dst, int dst_step, const void* d_map, int map_step, const uint8_t bg[4], const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, bg != nullptr && remap_plane_ok(d_map, map_step, rows, cols, 8) && c4_planes_ok(d_src, src_step, rows, cols, d_dst, dst_step, rows, cols));
    LVK_HIP_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(d_map) | (uintptr_t)map_step) & 7u) == 0);
    // (one kernel, no family to pick from: launched directly on the full grid; of `o` only the stream is read)
    hipLaunchKernelGGL(k_remap_map_c4, remap_grid(rows, c4_span(cols)), dim3(256), 0, o.stream, (const uint8_t*)d_src, src_step, rows, cols, (uint8_t*)d_dst, dst_step,
                       (const uint8_t*)d_map, map_step, pack_bg4(bg));
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// WarpMesh::apply on a four-channel frame: a 2 x 2 mesh goes through the homography kernel, anything larger through the mesh kernel
int lvk_launch_warpmesh_apply_lens_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                      const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4], const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, remap_mesh_ok(mesh, mesh_rows, mesh_cols));
    if (mesh_rows == 2 && mesh_cols == 2)
    {
        float H[9];
        lvkh::mesh2x2_to_homography(mesh, rows, cols, H);
        return lvk_launch_remap_homography_c4(ctx, d_src, src_step, rows, cols, d_dst, dst_step, rows, cols, 0, 0, H, bg, o);
    }
    return lvk_launch_remap_mesh_c4(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, o);
}

extern "C" {

int lvk_hip_remap_homography_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                                void* d_dst, int dst_step, int dst_rows, int dst_cols, int off_x, int off_y, const float H[9], const uint8_t bg[4])
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_remap_homography_c4(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, H, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_remap_mesh_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols, void* d_dst, int dst_step,
                          const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4])
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_remap_mesh_c4(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_remap_map_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                         const void* d_map, int map_step, const uint8_t bg[4])
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_remap_map_c4(ctx, d_src, src_step, rows, cols, d_dst, dst_step, d_map, map_step, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_warpmesh_apply_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                              const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4])
{
    LVK_HIP_ENTRY(ctx);
    LVK_HIP_REQUIRE(ctx, bg != nullptr);
    return lvk_launch_warpmesh_apply_lens_c4(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream});
}

int lvk_hip_warpmesh_apply_lens_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                   const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4], const lvk_camera_params* lens)
{
    LVK_HIP_ENTRY(ctx);
    LVK_HIP_REQUIRE(ctx, bg != nullptr && lens != nullptr && rows > 1 && cols > 1);
    LensModel m; LensArgs a;
    const int rc = lvk_lens_model_build(*lens, rows, cols, m);
    if (rc != LVK_HIP_OK) return ctx->fail(rc, "invalid camera profile");
    std::memcpy(a.f, m.f, sizeof(a.f));
    return lvk_launch_warpmesh_apply_lens_c4(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream, LVK_REMAP_EXACT, &a});
}

} // extern "C"
