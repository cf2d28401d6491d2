// Dense frame remap for gfx950, kernels and launchers: lvk::remap x2 (LiveVisionKit/Functions/Image.cpp:28-151), WarpMesh::apply
// (Math/WarpMesh.cpp:183-223), lvk::upscale (Image.cpp:155-202) and the fused remap + 4:2:0 egress of the plugin's path.  The EASU arithmetic, the
// coordinate generators, the sinks, the strip walk, the kernel bodies and the one launch path (launch_remap, with_staged_mesh) are in remap_core.hpp.
#include "remap_core.hpp"
#ifndef LVK_CO_LDS_PAD
#define LVK_CO_LDS_PAD 0
#endif

namespace {


// (each LVK_REMAP_KERNEL* below defines the exact kernel NAME and its 1-LSB twin NAME_r1 from one body; the bodies themselves, remap_homography and
//  LVK_WITH_MESH_COORD, serve the kernel with and the kernel without the lens pre-warp -- remap_core.hpp)
LVK_REMAP_KERNEL_CO(bool YUV, k_remap_homography,
                    (const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                     uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols,
                     int off_x, int off_y, HomographyArgs H, uint32_t bg),
{
    remap_homography<YUV, W, false>(src, src_step, src_rows, src_cols, PackedSink{dst, dst_step}, dst_rows, dst_cols, off_x, off_y, H, LensArgs{}, bg);
})

LVK_REMAP_KERNEL_CO(bool YUV, k_remap_homography_lens,
                    (const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                     uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols,
                     int off_x, int off_y, HomographyArgs H, LensArgs L, uint32_t bg),
{
    remap_homography<YUV, W, true>(src, src_step, src_rows, src_cols, PackedSink{dst, dst_step}, dst_rows, dst_cols, off_x, off_y, H, L, bg);
})

LVK_REMAP_KERNEL_CO(bool YUV, k_remap_mesh,
                    (const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                     uint8_t* __restrict__ dst, int dst_step,
                     const float* __restrict__ mesh, int mesh_cols, int mesh_floats,
                     const LinTabEntry* __restrict__ xtab, const LinTabEntry* __restrict__ ytab, uint32_t bg),
{
    LVK_WITH_MESH_COORD(false, LensArgs{}, src_rows, src_cols, (remap_strip<YUV, W>(src, src_step, src_rows, src_cols, PackedSink{dst, dst_step}, src_rows, src_cols, coord, bg)))
})

LVK_REMAP_KERNEL_CO(bool YUV, k_remap_mesh_lens,
                    (const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                     uint8_t* __restrict__ dst, int dst_step,
                     const float* __restrict__ mesh, int mesh_cols, int mesh_floats,
                     const LinTabEntry* __restrict__ xtab, const LinTabEntry* __restrict__ ytab, LensArgs L, uint32_t bg),
{
    LVK_WITH_MESH_COORD(true, L, src_rows, src_cols, (remap_strip<YUV, W>(src, src_step, src_rows, src_cols, PackedSink{dst, dst_step}, src_rows, src_cols, coord, bg)))
})

LVK_REMAP_KERNEL(bool YUV, , k_remap_map,
                 (const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                  uint8_t* __restrict__ dst, int dst_step, const uint8_t* __restrict__ map, int map_step, uint32_t bg),
{
    const MapCoord coord{map, map_step};
    remap_strip<YUV, W>(src, src_step, src_rows, src_cols, PackedSink{dst, dst_step}, src_rows, src_cols, coord, bg);
})

// lvk::upscale (Image.cpp:155-202): the same strip body; the source coordinate never leaves the image, so the border band is the
// nearest copy of FSR.cl:342-351 and the background is unreachable.  Exact in every remap precision: it has no 1-LSB twin.
template <bool YUV>
__global__ __launch_bounds__(256) LVK_REMAP_ATTR
void k_easu_scale(const uint8_t* __restrict__ src, int src_step, int src_rows, int src_cols,
                  uint8_t* __restrict__ dst, int dst_step, int dst_rows, int dst_cols, float rsx, float rsy)
{
    const ScaleCoord coord{rsx, rsy};
    remap_strip<YUV>(src, src_step, src_rows, src_cols, PackedSink{dst, dst_step}, dst_rows, dst_cols, coord, 0u);
}

// ---- remap + 4:2:0 egress in one kernel (lvk_hip_stab_push_yuv420): YUV frames only, same size in and out, occupancy-capped like
//      the other kernels the overlap mode runs next to the tracker
//      Planes420: yuv420::PlanesOut in the order these sixteen kernels have always taken their planes in.  It stays: with PlanesOut as the argument the
//      compiler groups the scalar argument loads differently and every one of them comes out with another instruction stream.
struct Planes420 { uint8_t* y; int ys; uint8_t* u; int us; uint8_t* v; int vs; };

LVK_REMAP_KERNEL(bool NV12, LVK_CO_SCHEDULED, k_remap_homography_420,
                 (const uint8_t* __restrict__ src, int src_step, int rows, int cols, Planes420 o, HomographyArgs H, uint32_t bg),
{
    LVK_TL(0);
    remap_homography<true, W, false>(src, src_step, rows, cols, sink420<NV12>(o), rows, cols, 0, 0, H, LensArgs{}, bg);
})

LVK_REMAP_KERNEL(bool NV12, LVK_CO_SCHEDULED, k_remap_homography_lens_420,
                 (const uint8_t* __restrict__ src, int src_step, int rows, int cols, Planes420 o, HomographyArgs H, LensArgs L, uint32_t bg),
{
    remap_homography<true, W, true>(src, src_step, rows, cols, sink420<NV12>(o), rows, cols, 0, 0, H, L, bg);
})

LVK_REMAP_KERNEL(bool NV12, LVK_CO_SCHEDULED, k_remap_mesh_420,
                 (const uint8_t* __restrict__ src, int src_step, int rows, int cols, Planes420 o,
                  const float* __restrict__ mesh, int mesh_cols, int mesh_floats, const LinTabEntry* __restrict__ xtab, const LinTabEntry* __restrict__ ytab, uint32_t bg),
{
    const Sink420<NV12> sink = sink420<NV12>(o);
    LVK_WITH_MESH_COORD(false, LensArgs{}, rows, cols, (remap_strip<true, W>(src, src_step, rows, cols, sink, rows, cols, coord, bg)))
})

LVK_REMAP_KERNEL(bool NV12, LVK_CO_SCHEDULED, k_remap_mesh_lens_420,
                 (const uint8_t* __restrict__ src, int src_step, int rows, int cols, Planes420 o,
                  const float* __restrict__ mesh, int mesh_cols, int mesh_floats, const LinTabEntry* __restrict__ xtab, const LinTabEntry* __restrict__ ytab,
                  LensArgs L, uint32_t bg),
{
    const Sink420<NV12> sink = sink420<NV12>(o);
    LVK_WITH_MESH_COORD(true, L, rows, cols, (remap_strip<true, W>(src, src_step, rows, cols, sink, rows, cols, coord, bg)))
})

} // namespace

int lvk_launch_remap_homography(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                                void* d_dst, int dst_step, int dst_rows, int dst_cols,
                                int off_x, int off_y, const float H[9], const uint8_t bg[3], int yuv, const RemapLaunch& o)
{
    // Image.cpp:93-98
    LVK_HIP_REQUIRE(ctx, remap_precision_known(o.precision));
    LVK_HIP_REQUIRE(ctx, H != nullptr && bg != nullptr);
    LVK_HIP_REQUIRE(ctx, remap_plane_ok(d_src, src_step, src_rows, src_cols, 3) && remap_plane_ok(d_dst, dst_step, dst_rows, dst_cols, 3));
    HomographyArgs args;
    std::memcpy(args.h, H, sizeof(args.h));
    if (o.lens)
        launch_remap(ctx, LVK_REMAP_FORMS_CO(k_remap_homography_lens, false, true), yuv != 0, dst_rows, dst_cols, o, 0, (const uint8_t*)d_src, src_step, src_rows, src_cols,
                     (uint8_t*)d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, args, *o.lens, pack_bg(bg));
    else
        launch_remap(ctx, LVK_REMAP_FORMS_CO(k_remap_homography, false, true), yuv != 0, dst_rows, dst_cols, o, 0, (const uint8_t*)d_src, src_step, src_rows, src_cols,
                     (uint8_t*)d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, args, pack_bg(bg));
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

int lvk_launch_remap_mesh(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                          void* d_dst, int dst_step,
                          const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3], int yuv, const RemapLaunch& o)
{
    // Image.cpp:30-34
    LVK_HIP_REQUIRE(ctx, remap_precision_known(o.precision));
    LVK_HIP_REQUIRE(ctx, bg != nullptr && remap_mesh_ok(mesh, mesh_rows, mesh_cols));
    LVK_HIP_REQUIRE(ctx, remap_plane_ok(d_src, src_step, src_rows, src_cols, 3) && remap_plane_ok(d_dst, dst_step, src_rows, src_cols, 3));
    return with_staged_mesh(ctx, o.stream, mesh, mesh_rows, mesh_cols, src_rows, src_cols, [&](const StagedMesh& m) {
        if (o.lens)
            launch_remap(ctx, LVK_REMAP_FORMS_CO(k_remap_mesh_lens, false, true), yuv != 0, src_rows, src_cols, o, 0, (const uint8_t*)d_src, src_step, src_rows, src_cols,
                         (uint8_t*)d_dst, dst_step, m.d_mesh, m.mesh_cols, m.mesh_floats, m.xtab, m.ytab, *o.lens, pack_bg(bg));
        else
            launch_remap(ctx, LVK_REMAP_FORMS_CO(k_remap_mesh, false, true), yuv != 0, src_rows, src_cols, o, 0, (const uint8_t*)d_src, src_step, src_rows, src_cols,
                         (uint8_t*)d_dst, dst_step, m.d_mesh, m.mesh_cols, m.mesh_floats, m.xtab, m.ytab, pack_bg(bg));
    });
}

// lvk::remap(src, dst, offset_map, background) with the map resident in HBM (Functions/Image.cpp:28-81): dst and map have
// the size of src (the path never uses map ROIs).  d_map: rows x cols float2 offsets in pixels, pitch map_step bytes.
int lvk_launch_remap_map(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                         void* d_dst, int dst_step, const void* d_map, int map_step, const uint8_t bg[3], int yuv, const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, remap_precision_known(o.precision));
    LVK_HIP_REQUIRE(ctx, bg != nullptr);                                                                 // Image.cpp:30-34
    LVK_HIP_REQUIRE(ctx, remap_plane_ok(d_src, src_step, rows, cols, 3) && remap_plane_ok(d_dst, dst_step, rows, cols, 3) && remap_map_ok(d_map, map_step, rows, cols));
    // (a materialised map has no lens form and no persistent grid: of `o` the stream and the precision are read)
    launch_remap(ctx, LVK_REMAP_FORMS(k_remap_map, false, true), yuv != 0, rows, cols, RemapLaunch{o.stream, o.precision}, 0, (const uint8_t*)d_src, src_step, rows, cols, (uint8_t*)d_dst, dst_step,
                 (const uint8_t*)d_map, map_step, pack_bg(bg));
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// lvk::upscale(src, dst, size, yuv) (Functions/Image.cpp:155-202)
int lvk_launch_upscale(lvk_hip_ctx* ctx, hipStream_t stream, const void* d_src, int src_step, int src_rows, int src_cols,
                       void* d_dst, int dst_step, int dst_rows, int dst_cols, int yuv)
{
    LVK_HIP_REQUIRE(ctx, d_src != d_dst);
    LVK_HIP_REQUIRE(ctx, dst_cols >= src_cols && dst_rows >= src_rows);                         // Image.cpp:157
    LVK_HIP_REQUIRE(ctx, remap_plane_ok(d_src, src_step, src_rows, src_cols, 3) && remap_plane_ok(d_dst, dst_step, dst_rows, dst_cols, 3));   // Image.cpp:158
    if (dst_cols == src_cols && dst_rows == src_rows)                                           // Image.cpp:162-166
    {
        LVK_HIP_CHECK(ctx, hipMemcpy2DAsync(d_dst, (size_t)dst_step, d_src, (size_t)src_step, 3 * (size_t)src_cols, (size_t)src_rows,
                                            hipMemcpyDeviceToDevice, stream));
        return LVK_HIP_OK;
    }
    const float rsx = (float)src_cols / (float)dst_cols, rsy = (float)src_rows / (float)dst_rows;
    const dim3 block(256), grid = remap_grid(dst_rows, dst_cols);
    if (yuv) hipLaunchKernelGGL(k_easu_scale<true>, grid, block, 0, stream, (const uint8_t*)d_src, src_step, src_rows, src_cols, (uint8_t*)d_dst, dst_step, dst_rows, dst_cols, rsx, rsy);
    else hipLaunchKernelGGL(k_easu_scale<false>, grid, block, 0, stream, (const uint8_t*)d_src, src_step, src_rows, src_cols, (uint8_t*)d_dst, dst_step, dst_rows, dst_cols, rsx, rsy);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

int lvk_launch_warpmesh_apply_lens(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                                   void* d_dst, int dst_step,
                                   const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3], int yuv, const RemapLaunch& o)
{
    return route_warpmesh(ctx, mesh, mesh_rows, mesh_cols, rows, cols,
                          [&](const float H[9]) { return lvk_launch_remap_homography(ctx, d_src, src_step, rows, cols, d_dst, dst_step, rows, cols, 0, 0, H, bg, yuv, o); },
                          [&] { return lvk_launch_remap_mesh(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, yuv, o); });
}

// WarpMesh::apply + I4XXIngest / NV12Ingest::to_obs in one launch: d_src packed YUV 8UC3, output planar 4:2:0 (I420: y, u, v; NV12: y, uv).
int lvk_launch_warpmesh_apply_420(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                                  void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int nv12,
                                  const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3], const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, remap_precision_known(o.precision));
    LVK_HIP_REQUIRE(ctx, bg != nullptr && remap_mesh_ok(mesh, mesh_rows, mesh_cols));
    const yuv420::PlaneSet dst = yuv420::plane_set(o_y, oy_step, o_u, ou_step, o_v, ov_step, nv12, rows, cols);
    LVK_HIP_REQUIRE(ctx, remap_plane_ok(d_src, src_step, rows, cols, 3) && yuv420::well_formed(dst, true));
    const yuv420::PlanesOut po = dst.out();
    const Planes420 planes{po.y, po.ys, po.u, po.us, po.v, po.vs};
    const size_t lds_pad = o.co_scheduled ? (size_t)LVK_CO_LDS_PAD : 0;          // A / B switch (scripts/variant_build.sh): unused LDS that caps the persistent grid's blocks per CU
    if (mesh_rows == 2 && mesh_cols == 2)
    {
        HomographyArgs H;
        lvkh::mesh2x2_to_homography(mesh, rows, cols, H.h);
        if (o.lens) launch_remap(ctx, LVK_REMAP_FORMS(k_remap_homography_lens_420, false, true), nv12 != 0, rows, cols, o, lds_pad, (const uint8_t*)d_src, src_step, rows, cols, planes, H, *o.lens, pack_bg(bg));
        else launch_remap(ctx, LVK_REMAP_FORMS(k_remap_homography_420, false, true), nv12 != 0, rows, cols, o, lds_pad, (const uint8_t*)d_src, src_step, rows, cols, planes, H, pack_bg(bg));
        LVK_HIP_CHECK(ctx, hipGetLastError());
        return LVK_HIP_OK;
    }
    return with_staged_mesh(ctx, o.stream, mesh, mesh_rows, mesh_cols, rows, cols, [&](const StagedMesh& m) {
        if (o.lens) launch_remap(ctx, LVK_REMAP_FORMS(k_remap_mesh_lens_420, false, true), nv12 != 0, rows, cols, o, lds_pad, (const uint8_t*)d_src, src_step, rows, cols, planes,
                                 m.d_mesh, m.mesh_cols, m.mesh_floats, m.xtab, m.ytab, *o.lens, pack_bg(bg));
        else launch_remap(ctx, LVK_REMAP_FORMS(k_remap_mesh_420, false, true), nv12 != 0, rows, cols, o, lds_pad, (const uint8_t*)d_src, src_step, rows, cols, planes,
                          m.d_mesh, m.mesh_cols, m.mesh_floats, m.xtab, m.ytab, pack_bg(bg));
    });
}

extern "C" {

int lvk_hip_remap_homography(lvk_hip_ctx* ctx,
                             const void* d_src, int src_step, int src_rows, int src_cols,
                             void* d_dst, int dst_step, int dst_rows, int dst_cols,
                             int off_x, int off_y, const float H[9], const uint8_t bg[3], int yuv)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_remap_homography(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols, off_x, off_y, H, bg, yuv, RemapLaunch{ctx->stream, ctx->remap_precision});
}

int lvk_hip_remap_mesh(lvk_hip_ctx* ctx,
                       const void* d_src, int src_step, int src_rows, int src_cols,
                       void* d_dst, int dst_step,
                       const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3], int yuv)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_remap_mesh(ctx, d_src, src_step, src_rows, src_cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, yuv, RemapLaunch{ctx->stream, ctx->remap_precision});
}

int lvk_hip_remap_map(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                      const void* d_map, int map_step, const uint8_t bg[3], int yuv)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_remap_map(ctx, d_src, src_step, rows, cols, d_dst, dst_step, d_map, map_step, bg, yuv, RemapLaunch{ctx->stream, ctx->remap_precision});
}

int lvk_hip_warpmesh_apply_lens(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3], int yuv, const lvk_camera_params* lens)
{
    LVK_HIP_ENTRY(ctx);
    LVK_HIP_REQUIRE(ctx, lens != nullptr && rows > 1 && cols > 1);
    LensArgs a;
    const int rc = lens_args_of(ctx, lens, rows, cols, a);
    if (rc != LVK_HIP_OK) return rc;
    return lvk_launch_warpmesh_apply_lens(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, yuv, RemapLaunch{ctx->stream, ctx->remap_precision, &a});
}

int lvk_hip_warpmesh_apply_yuv420(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                                  void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int nv12,
                                  const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3])
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_warpmesh_apply_420(ctx, d_src, src_step, rows, cols, o_y, oy_step, o_u, ou_step, o_v, ov_step, nv12, mesh, mesh_rows, mesh_cols, bg, RemapLaunch{ctx->stream, ctx->remap_precision});
}

int lvk_hip_upscale(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                    void* d_dst, int dst_step, int dst_rows, int dst_cols, int yuv)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_upscale(ctx, ctx->stream, d_src, src_step, src_rows, src_cols, d_dst, dst_step, dst_rows, dst_cols, yuv);
}

int lvk_hip_warpmesh_apply(lvk_hip_ctx* ctx,
                           const void* d_src, int src_step, int rows, int cols,
                           void* d_dst, int dst_step,
                           const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3], int yuv)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_launch_warpmesh_apply_lens(ctx, d_src, src_step, rows, cols, d_dst, dst_step, mesh, mesh_rows, mesh_cols, bg, yuv, RemapLaunch{ctx->stream, ctx->remap_precision});
}

} // extern "C"

LVK_TL_EXPORT(remap)
