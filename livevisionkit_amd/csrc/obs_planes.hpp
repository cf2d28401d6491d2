// The planes of the OBS video formats as the entries that take "every format FrameIngest::Select accepts" describe them (lvk_hip_lens_apply_obs,
// lvk_hip_remap_map_obs, lvk_hip_scale_obs, lvk_hip_deblock_apply_obs, lvk_hip_cas_obs, lvk_hip_fsr_obs): which formats are 4:2:0, the planes of the others and the bytes of their rows, the
// parity of a frame size, the byte spans of a frame's planes, and the routes lvk_hip_scale_obs, lvk_hip_deblock_apply_obs, lvk_hip_cas_obs and lvk_hip_fsr_obs
// take.  Plain C++ on top of planes420.hpp, no HIP: tests/cpp/obs_planes_check.cpp, tests/cpp/deblock_route_check.cpp, tests/cpp/cas_route_check.cpp and
// tests/cpp/fsr_route_check.cpp compile it on the CPU.
#pragma once

#include "planes420.hpp"
#include "lvk_hip.h"

namespace obs {

using namespace yuv420;

inline bool is_420(int vf) { return vf == LVK_VIDEO_FORMAT_I420 || vf == LVK_VIDEO_FORMAT_I40A || vf == LVK_VIDEO_FORMAT_NV12; }
inline PlaneSet plane_set_420(int vf, const void* const p[3], const int s[3], int rows, int cols)
{
    return plane_set(p[0], s[0], p[1], s[1], p[2], s[2], vf == LVK_VIDEO_FORMAT_NV12 ? 1 : 0, rows, cols);
}

// The planes FrameIngest moves for one rows x cols frame of a format outside 4:2:0: their number and the bytes of a row (every plane has `rows` rows).
// The 4-byte DirectIngest formats are the tight plane of 4 * cols bytes a row of which rows * cols * 3 bytes move.  0 planes: no such format.
struct ObsRows { int n; int bytes[3]; };
inline ObsRows obs_rows(int vf, int cols)
{
    switch (vf)
    {
    case LVK_VIDEO_FORMAT_I422: case LVK_VIDEO_FORMAT_I42A: return {3, {cols, cols / 2, cols / 2}};
    case LVK_VIDEO_FORMAT_I444: case LVK_VIDEO_FORMAT_YUVA: return {3, {cols, cols, cols}};
    case LVK_VIDEO_FORMAT_YUY2: case LVK_VIDEO_FORMAT_YVYU: case LVK_VIDEO_FORMAT_UYVY: return {1, {2 * cols, 0, 0}};
    case LVK_VIDEO_FORMAT_AYUV: case LVK_VIDEO_FORMAT_RGBA: case LVK_VIDEO_FORMAT_BGRA: case LVK_VIDEO_FORMAT_BGRX: return {1, {4 * cols, 0, 0}};
    case LVK_VIDEO_FORMAT_BGR3: return {1, {3 * cols, 0, 0}};
    case LVK_VIDEO_FORMAT_Y800: return {1, {cols, 0, 0}};
    default: return {0, {0, 0, 0}};
    }
}
inline bool is_direct4(int vf) { return vf == LVK_VIDEO_FORMAT_RGBA || vf == LVK_VIDEO_FORMAT_BGRA || vf == LVK_VIDEO_FORMAT_BGRX; }
inline bool is_422(int vf)
{
    return vf == LVK_VIDEO_FORMAT_I422 || vf == LVK_VIDEO_FORMAT_I42A || vf == LVK_VIDEO_FORMAT_YUY2 || vf == LVK_VIDEO_FORMAT_YVYU || vf == LVK_VIDEO_FORMAT_UYVY;
}

// the parity FrameIngest asks of a frame size: even cols on 4:2:2, even rows and cols on 4:2:0; both positive
inline bool obs_size_ok(int vf, int rows, int cols)
{
    if (rows <= 0 || cols <= 0) return false;
    if (is_420(vf)) return ((rows | cols) & 1) == 0;
    return !is_422(vf) || (cols & 1) == 0;
}

// The spans of the planes of a format outside 4:2:0 (every plane there, every pitch at least its row: the caller has checked).  The 4-byte DirectIngest
// formats span their whole tight plane, of which the last quarter is neither read nor written.
inline Spans obs_spans(int vf, const void* const planes[3], const int steps[3], int rows, int cols)
{
    const ObsRows t = obs_rows(vf, cols);
    Spans s{{}, t.n};
    for (int i = 0; i < t.n; i++) s.s[i] = span_of(planes[i], steps[i], rows, t.bytes[i]);
    return s;
}

// lvk_hip_scale_obs: the launches behind one call, by format and by whether the two sizes are equal
enum class ScaleRoute
{
    None,           // not a format FrameIngest::Select knows
    Planes420,      // the body of lvk_hip_scale_yuv420
    FusedPlanes,    // k_rcas_obs<PlaneSrc>: one launch, planes to planes
    FusedPacked,    // ingest -> EASU (yuv) -> k_rcas_obs<PackedSrc>
    Bgr,            // [EASU (not yuv) ->] RCAS on three-byte pixels: BGR3 at its pitch, RGBA / BGRA / BGRX on the 3 * cols view
    Gray            // [gray EASU ->] gray RCAS
};

inline ScaleRoute scale_route(int vf, bool equal_sizes)
{
    if (is_420(vf)) return ScaleRoute::Planes420;
    if (vf == LVK_VIDEO_FORMAT_Y800) return ScaleRoute::Gray;
    if (vf == LVK_VIDEO_FORMAT_BGR3 || is_direct4(vf)) return ScaleRoute::Bgr;
    if (obs_rows(vf, 2).n == 0) return ScaleRoute::None;
    return equal_sizes ? ScaleRoute::FusedPlanes : ScaleRoute::FusedPacked;
}

// lvk_hip_deblock_apply_obs: the launches behind one call, by format
enum class DeblockRoute
{
    None,           // not a format FrameIngest::Select knows
    Planes420,      // the body of lvk_hip_deblock_apply_yuv420
    Fused,          // statistics on the luma, downscale from the planes, median, blend into the planes: no packed frame (4:2:2, 4:4:4, AYUV)
    Bgr,            // a copy, then the packed three-channel apply in place on the output: BGR3 at its pitch, RGBA / BGRA / BGRX on the 3 * cols view
    Gray            // a copy, then the gray apply in place on the output plane
};

inline DeblockRoute deblock_route(int vf)
{
    if (is_420(vf)) return DeblockRoute::Planes420;
    if (vf == LVK_VIDEO_FORMAT_Y800) return DeblockRoute::Gray;
    if (vf == LVK_VIDEO_FORMAT_BGR3 || is_direct4(vf)) return DeblockRoute::Bgr;
    return obs_rows(vf, 2).n == 0 ? DeblockRoute::None : DeblockRoute::Fused;
}

// lvk_hip_cas_obs: the launch behind one call, by format
enum class CasRoute
{
    None,           // not a format FrameIngest::Select knows
    Planes420,      // the body of lvk_hip_cas_yuv420: k_cas_420
    Fused,          // k_cas_obs<Src, Sink>: one launch, planes to planes (4:2:2, 4:4:4, AYUV)
    Bgr,            // lvk_hip_cas on three-byte pixels, plane to plane: BGR3 at its pitch, RGBA / BGRA / BGRX on the 3 * cols view
    Gray            // lvk_hip_cas_gray, plane to plane
};

inline CasRoute cas_route(int vf)
{
    if (is_420(vf)) return CasRoute::Planes420;
    if (vf == LVK_VIDEO_FORMAT_Y800) return CasRoute::Gray;
    if (vf == LVK_VIDEO_FORMAT_BGR3 || is_direct4(vf)) return CasRoute::Bgr;
    return obs_rows(vf, 2).n == 0 ? CasRoute::None : CasRoute::Fused;
}

// lvk_hip_fsr_obs: the launches behind one call, by format and by whether the tile's source footprint fits the LDS stage (lvk_hip_fsr_obs_path;
// DESIGN.md section 33)
enum class FsrRoute
{
    None,           // not a format FrameIngest::Select knows
    Planes420,      // the body of lvk_hip_fsr_yuv420: k_fsr_planes staged from the planes, or ingest into a pooled frame and its direct taps
    FusedPlanes,    // k_fsr_planes<plane source, sink, staged>: one launch, planes to planes (4:2:2, 4:4:4, AYUV)
    FusedPacked,    // ingest into a pooled frame -> k_fsr_planes<PackedYuv, sink, direct> into the planes
    Bgr,            // lvk_hip_fsr_easu on three-byte pixels, plane to plane: BGR3 at its pitches, RGBA / BGRA / BGRX on the 3 * cols views
    Gray            // lvk_hip_fsr_easu_gray, plane to plane
};

inline FsrRoute fsr_route(int vf, bool staged)
{
    if (is_420(vf)) return FsrRoute::Planes420;
    if (vf == LVK_VIDEO_FORMAT_Y800) return FsrRoute::Gray;
    if (vf == LVK_VIDEO_FORMAT_BGR3 || is_direct4(vf)) return FsrRoute::Bgr;
    if (obs_rows(vf, 2).n == 0) return FsrRoute::None;
    return staged ? FsrRoute::FusedPlanes : FsrRoute::FusedPacked;
}

// Where the luma bytes of a row of a fused format lie: the first at byte `first`, the next `stride` bytes on.  Planar Y planes: {0, 1}.
struct LumaBytes { int first, stride; };
inline LumaBytes luma_bytes(int vf)
{
    switch (vf)
    {
    case LVK_VIDEO_FORMAT_YUY2: case LVK_VIDEO_FORMAT_YVYU: return {0, 2};
    case LVK_VIDEO_FORMAT_UYVY: return {1, 2};
    case LVK_VIDEO_FORMAT_AYUV: return {1, 4};
    default: return {0, 1};
    }
}

} // namespace obs
