// Remap + egress in one kernel for the OBS video formats that are not 4:2:0 (lvk_hip_stab_push_obs): the EASU remap of remap_core.hpp with a sink that
// writes the frame the way FrameIngest::to_obs would (reference: Modules/OBS-Plugin/Interop/FrameIngest.cpp:526-557 I4XXIngest, :640-666 P422Ingest,
// :690-703 P444Ingest) -- planar or packed 4:2:2 (chroma = cv::resize(0.5, 1.0, INTER_AREA) = the pixel pair's mean, round half to even), planar 4:4:4,
// AYUV.  Same bytes as lvk_launch_warpmesh_apply_lens followed by lvk_launch_egress_obs (tests/test_ingest_obs_gpu.py holds the two routes together);
// what it saves is the packed intermediate (2 x 3 W H bytes), one kernel and one launch per frame.  The same sinks behind a materialised offset map
// (k_remap_map_planes, lvk_launch_remap_map_obs) are the lens filter's remap + egress on these formats: lvk_hip_remap_map_obs, DESIGN.md section 29.
#include "remap_core.hpp"
#include "obs_sinks.hpp"

namespace {

// (each LVK_REMAP_KERNEL below defines the exact kernel NAME and its 1-LSB twin NAME_r1 from one body; remap_homography and LVK_WITH_MESH_COORD are the bodies of
//  the kernels with and without the lens pre-warp -- remap_core.hpp)
LVK_REMAP_KERNEL(class Sink, LVK_CO_SCHEDULED, k_remap_homography_planes,
                 (const uint8_t* __restrict__ src, int src_step, int rows, int cols, Sink sink, HomographyArgs H, uint32_t bg),
{
    remap_homography<true, W, false>(src, src_step, rows, cols, sink, rows, cols, 0, 0, H, LensArgs{}, bg);
})

LVK_REMAP_KERNEL(class Sink, LVK_CO_SCHEDULED, k_remap_homography_lens_planes,
                 (const uint8_t* __restrict__ src, int src_step, int rows, int cols, Sink sink, HomographyArgs H, LensArgs L, uint32_t bg),
{
    remap_homography<true, W, true>(src, src_step, rows, cols, sink, rows, cols, 0, 0, H, L, bg);
})

LVK_REMAP_KERNEL(class Sink, LVK_CO_SCHEDULED, k_remap_mesh_planes,
                 (const uint8_t* __restrict__ src, int src_step, int rows, int cols, Sink sink,
                  const float* __restrict__ mesh, int mesh_cols, int mesh_floats, const LinTabEntry* __restrict__ xtab, const LinTabEntry* __restrict__ ytab, uint32_t bg),
{
    LVK_WITH_MESH_COORD(false, LensArgs{}, rows, cols, (remap_strip<true, W>(src, src_step, rows, cols, sink, rows, cols, coord, bg)))
})

LVK_REMAP_KERNEL(class Sink, LVK_CO_SCHEDULED, k_remap_mesh_lens_planes,
                 (const uint8_t* __restrict__ src, int src_step, int rows, int cols, Sink sink,
                  const float* __restrict__ mesh, int mesh_cols, int mesh_floats, const LinTabEntry* __restrict__ xtab, const LinTabEntry* __restrict__ ytab,
                  LensArgs L, uint32_t bg),
{
    LVK_WITH_MESH_COORD(true, L, rows, cols, (remap_strip<true, W>(src, src_step, rows, cols, sink, rows, cols, coord, bg)))
})

// Full grid only, as k_remap_map_420: a materialised map has no persistent-grid form (lvk_launch_remap_map)
LVK_REMAP_KERNEL(class Sink, , k_remap_map_planes,
                 (const uint8_t* __restrict__ src, int src_step, int rows, int cols, Sink sink, const uint8_t* __restrict__ map, int map_step, uint32_t bg),
{
    remap_strip<true, W>(src, src_step, rows, cols, sink, rows, cols, MapCoord{map, map_step}, bg);
})

// (the family's "flag" is the sink type: one form per precision)
template <class Sink>
int launch_planes(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, const Sink& sink,
                  const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3], const RemapLaunch& o)
{
    if (mesh_rows == 2 && mesh_cols == 2)
    {
        HomographyArgs H;
        lvkh::mesh2x2_to_homography(mesh, rows, cols, H.h);
        if (o.lens) launch_remap(ctx, LVK_REMAP_FORMS(k_remap_homography_lens_planes, Sink, Sink), false, rows, cols, o, 0, (const uint8_t*)d_src, src_step, rows, cols, sink, H, *o.lens, pack_bg(bg));
        else launch_remap(ctx, LVK_REMAP_FORMS(k_remap_homography_planes, Sink, Sink), false, rows, cols, o, 0, (const uint8_t*)d_src, src_step, rows, cols, sink, H, pack_bg(bg));
        LVK_HIP_CHECK(ctx, hipGetLastError());
        return LVK_HIP_OK;
    }
    return with_staged_mesh(ctx, o.stream, mesh, mesh_rows, mesh_cols, rows, cols, [&](const StagedMesh& m) {
        if (o.lens) launch_remap(ctx, LVK_REMAP_FORMS(k_remap_mesh_lens_planes, Sink, Sink), false, rows, cols, o, 0, (const uint8_t*)d_src, src_step, rows, cols, sink,
                                 m.d_mesh, m.mesh_cols, m.mesh_floats, m.xtab, m.ytab, *o.lens, pack_bg(bg));
        else launch_remap(ctx, LVK_REMAP_FORMS(k_remap_mesh_planes, Sink, Sink), false, rows, cols, o, 0, (const uint8_t*)d_src, src_step, rows, cols, sink,
                          m.d_mesh, m.mesh_cols, m.mesh_floats, m.xtab, m.ytab, pack_bg(bg));
    });
}

} // namespace

bool lvk_remap_obs_fusable(int video_format)
{
    switch (video_format)
    {
    case LVK_VIDEO_FORMAT_I422: case LVK_VIDEO_FORMAT_I42A: case LVK_VIDEO_FORMAT_YUY2: case LVK_VIDEO_FORMAT_YVYU: case LVK_VIDEO_FORMAT_UYVY:
    case LVK_VIDEO_FORMAT_I444: case LVK_VIDEO_FORMAT_YUVA: case LVK_VIDEO_FORMAT_AYUV: return true;
    default: return false;
    }
}

// WarpMesh::apply + FrameIngest::to_obs of `video_format` in one kernel; the planes' geometry has been checked by the caller (lvk_stab_push_planes).
int lvk_launch_warpmesh_apply_obs(lvk_hip_ctx* ctx, int video_format, const void* d_src, int src_step, int rows, int cols,
                                  void* const planes[3], const int steps[3], const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3], const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, remap_precision_known(o.precision));
    LVK_HIP_REQUIRE(ctx, planes && steps && bg && remap_mesh_ok(mesh, mesh_rows, mesh_cols) && remap_plane_ok(d_src, src_step, rows, cols, 3));
    return with_obs_sink(ctx, "lvk_launch_warpmesh_apply_obs", video_format, rows, cols, planes, steps,
                         [&](const auto& sink) { return launch_planes(ctx, d_src, src_step, rows, cols, sink, mesh, mesh_rows, mesh_cols, bg, o); });
}

// lvk::remap(offset map) + FrameIngest::to_obs of `video_format` in one kernel: d_src packed YUV 8UC3, d_map rows x cols float2.  Of `o` the stream and
// the precision are read (lvk_launch_remap_map).  The caller has checked that no output plane overlaps the source, the map or another output plane.
int lvk_launch_remap_map_obs(lvk_hip_ctx* ctx, int video_format, const void* d_src, int src_step, int rows, int cols,
                             void* const planes[3], const int steps[3], const void* d_map, int map_step, const uint8_t bg[3], const RemapLaunch& o)
{
    LVK_HIP_REQUIRE(ctx, remap_precision_known(o.precision));
    LVK_HIP_REQUIRE(ctx, planes && steps && bg && remap_map_ok(d_map, map_step, rows, cols) && remap_plane_ok(d_src, src_step, rows, cols, 3));
    return with_obs_sink(ctx, "lvk_launch_remap_map_obs", video_format, rows, cols, planes, steps, [&](const auto& sink) {
        using Sink = std::decay_t<decltype(sink)>;
        launch_remap(ctx, LVK_REMAP_FORMS(k_remap_map_planes, Sink, Sink), false, rows, cols, RemapLaunch{o.stream, o.precision}, 0,
                     (const uint8_t*)d_src, src_step, rows, cols, sink, (const uint8_t*)d_map, map_step, pack_bg(bg));
        LVK_HIP_CHECK(ctx, hipGetLastError());
        return (int)LVK_HIP_OK;
    });
}
