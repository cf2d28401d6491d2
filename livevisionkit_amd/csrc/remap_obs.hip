// Remap + egress in one kernel for the OBS video formats that are not 4:2:0 (lvk_hip_stab_push_obs): the EASU remap of remap_core.hpp with a sink that
// writes the frame the way FrameIngest::to_obs would (reference: Modules/OBS-Plugin/Interop/FrameIngest.cpp:526-557 I4XXIngest, :640-666 P422Ingest,
// :690-703 P444Ingest) -- planar or packed 4:2:2 (chroma = cv::resize(0.5, 1.0, INTER_AREA) = the pixel pair's mean, round half to even), planar 4:4:4,
// AYUV.  Same bytes as lvk_launch_warpmesh_apply_lens followed by lvk_launch_egress_obs (tests/test_ingest_obs_gpu.py holds the two routes together);
// what it saves is the packed intermediate (2 x 3 W H bytes), one kernel and one launch per frame.  The same sinks behind a materialised offset map
// (k_remap_map_planes, lvk_launch_remap_map_obs) are the lens filter's remap + egress on these formats: lvk_hip_remap_map_obs, DESIGN.md section 29.
#include "remap_core.hpp"

namespace {

__device__ __forceinline__ uint32_t half_even_u32(uint32_t s) { return (s + ((s >> 1) & 1u)) >> 1; }      // cvRound(s * 0.5f)

// LAYOUT 0: planes Y, U, V (I422 / I42A); 1 YUY2 (Y U Y V); 2 YVYU; 3 UYVY.  A thread holds 4 horizontally adjacent pixels = 2 chroma pairs; the frame's
// width is even, so a thread at the right edge holds 2 or 4.
template <int LAYOUT>
struct Sink422
{
    uint8_t* __restrict__ p0; int s0; uint8_t* __restrict__ p1; int s1; uint8_t* __restrict__ p2; int s2;
    __device__ __forceinline__ void store(int x0, int y, int npx, const uint32_t px[PXT], bool active, int /*parity*/) const
    {
        if (!active) return;
        const uint32_t u0 = half_even_u32(((px[0] >> 8) & 0xffu) + ((px[1] >> 8) & 0xffu)), u1 = half_even_u32(((px[2] >> 8) & 0xffu) + ((px[3] >> 8) & 0xffu));
        const uint32_t v0 = half_even_u32(((px[0] >> 16) & 0xffu) + ((px[1] >> 16) & 0xffu)), v1 = half_even_u32(((px[2] >> 16) & 0xffu) + ((px[3] >> 16) & 0xffu));
        const uint32_t y0 = px[0] & 0xffu, y1 = px[1] & 0xffu, y2 = px[2] & 0xffu, y3 = px[3] & 0xffu;
        if (LAYOUT == 0)
        {
            uint8_t* yr = p0 + (__umul24((uint32_t)y, (uint32_t)s0) + (uint32_t)x0);
            uint8_t* ur = p1 + (__umul24((uint32_t)y, (uint32_t)s1) + (uint32_t)(x0 >> 1));
            uint8_t* vr = p2 + (__umul24((uint32_t)y, (uint32_t)s2) + (uint32_t)(x0 >> 1));
            const uint32_t yy = y0 | (y1 << 8) | (y2 << 16) | (y3 << 24);
            if (npx == PXT && ((reinterpret_cast<uintptr_t>(yr) & 3u) == 0)) LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(yr), yy);
            else for (int p = 0; p < npx; p++) yr[p] = (uint8_t)(yy >> (8 * p));
            ur[0] = (uint8_t)u0; vr[0] = (uint8_t)v0;
            if (npx > 2) { ur[1] = (uint8_t)u1; vr[1] = (uint8_t)v1; }
        }
        else
        {
            const uint32_t f0 = LAYOUT != 2 ? u0 : v0, g0 = LAYOUT != 2 ? v0 : u0, f1 = LAYOUT != 2 ? u1 : v1, g1 = LAYOUT != 2 ? v1 : u1;
            const uint32_t a = LAYOUT == 3 ? (f0 | (y0 << 8) | (g0 << 16) | (y1 << 24)) : (y0 | (f0 << 8) | (y1 << 16) | (g0 << 24));
            const uint32_t b = LAYOUT == 3 ? (f1 | (y2 << 8) | (g1 << 16) | (y3 << 24)) : (y2 | (f1 << 8) | (y3 << 16) | (g1 << 24));
            uint8_t* d = p0 + (__umul24((uint32_t)y, (uint32_t)s0) + 2u * (uint32_t)x0);
            if ((reinterpret_cast<uintptr_t>(d) & 3u) == 0)
            {
                LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(d), a);
                if (npx > 2) LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(d) + 1, b);
            }
            else
                for (int k = 0; k < 2 * npx; k++) d[k] = (uint8_t)((k < 4 ? a : b) >> (8 * (k & 3)));
        }
    }
};

// LAYOUT 0: planes Y, U, V (I444 / YUVA); 1: A Y U V with A = 255 (AYUV)
template <int LAYOUT>
struct Sink444
{
    uint8_t* __restrict__ p0; int s0; uint8_t* __restrict__ p1; int s1; uint8_t* __restrict__ p2; int s2;
    __device__ __forceinline__ void store(int x0, int y, int npx, const uint32_t px[PXT], bool active, int /*parity*/) const
    {
        if (!active) return;
        if (LAYOUT == 0)
        {
            uint8_t* r[3] = {p0 + (__umul24((uint32_t)y, (uint32_t)s0) + (uint32_t)x0), p1 + (__umul24((uint32_t)y, (uint32_t)s1) + (uint32_t)x0),
                             p2 + (__umul24((uint32_t)y, (uint32_t)s2) + (uint32_t)x0)};
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
            {
                const uint32_t w = ((px[0] >> (8 * ch)) & 0xffu) | (((px[1] >> (8 * ch)) & 0xffu) << 8) | (((px[2] >> (8 * ch)) & 0xffu) << 16) | (((px[3] >> (8 * ch)) & 0xffu) << 24);
                if (npx == PXT && ((reinterpret_cast<uintptr_t>(r[ch]) & 3u) == 0)) LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(r[ch]), w);
                else for (int p = 0; p < npx; p++) r[ch][p] = (uint8_t)(w >> (8 * p));
            }
        }
        else
        {
            uint8_t* d = p0 + (__umul24((uint32_t)y, (uint32_t)s0) + 4u * (uint32_t)x0);
            const bool al = (reinterpret_cast<uintptr_t>(d) & 3u) == 0;
            for (int p = 0; p < npx; p++)
            {
                const uint32_t w = 255u | (px[p] << 8);
                if (al) LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(d) + p, w);
                else { d[4 * p] = 255; d[4 * p + 1] = (uint8_t)px[p]; d[4 * p + 2] = (uint8_t)(px[p] >> 8); d[4 * p + 3] = (uint8_t)(px[p] >> 16); }
            }
        }
    }
};

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

// The sink of `video_format` over the caller's planes, checked, handed to launch(sink): the one switch of the two launchers below.  Plane i holds
// rows x `c` samples of `bpp` bytes; 4:2:2 has an even width.
template <class Launch>
int with_obs_sink(lvk_hip_ctx* ctx, const char* who, int video_format, int rows, int cols, void* const planes[3], const int steps[3], const Launch& launch)
{
    uint8_t* p0 = (uint8_t*)planes[0]; uint8_t* p1 = (uint8_t*)planes[1]; uint8_t* p2 = (uint8_t*)planes[2];
    auto plane_ok = [&](int i, int c, int bpp) { return remap_plane_ok(planes[i], steps[i], rows, c, bpp); };
    switch (video_format)
    {
    case LVK_VIDEO_FORMAT_I422: case LVK_VIDEO_FORMAT_I42A:
        LVK_HIP_REQUIRE(ctx, (cols & 1) == 0 && plane_ok(0, cols, 1) && plane_ok(1, cols / 2, 1) && plane_ok(2, cols / 2, 1));
        return launch(Sink422<0>{p0, steps[0], p1, steps[1], p2, steps[2]});
    case LVK_VIDEO_FORMAT_YUY2:
        LVK_HIP_REQUIRE(ctx, (cols & 1) == 0 && plane_ok(0, cols, 2));
        return launch(Sink422<1>{p0, steps[0], p0, 0, p0, 0});
    case LVK_VIDEO_FORMAT_YVYU:
        LVK_HIP_REQUIRE(ctx, (cols & 1) == 0 && plane_ok(0, cols, 2));
        return launch(Sink422<2>{p0, steps[0], p0, 0, p0, 0});
    case LVK_VIDEO_FORMAT_UYVY:
        LVK_HIP_REQUIRE(ctx, (cols & 1) == 0 && plane_ok(0, cols, 2));
        return launch(Sink422<3>{p0, steps[0], p0, 0, p0, 0});
    case LVK_VIDEO_FORMAT_I444: case LVK_VIDEO_FORMAT_YUVA:
        LVK_HIP_REQUIRE(ctx, plane_ok(0, cols, 1) && plane_ok(1, cols, 1) && plane_ok(2, cols, 1));
        return launch(Sink444<0>{p0, steps[0], p1, steps[1], p2, steps[2]});
    case LVK_VIDEO_FORMAT_AYUV:
        LVK_HIP_REQUIRE(ctx, plane_ok(0, cols, 4));
        return launch(Sink444<1>{p0, steps[0], p0, 0, p0, 0});
    }
    return ctx->fail(LVK_HIP_ERR_ARG, std::string(who) + ": no fused sink for video format " + std::to_string(video_format));
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
