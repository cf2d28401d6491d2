// lvk::FSRFilter on the planes of EVERY video format FrameIngest::Select accepts, out of place, in one call: lvk_hip_fsr_obs.
// The output planes are, byte for byte, those of
//   lvk_hip_ingest_obs -> lvk_hip_fsr_easu(format = lvk_hip_obs_frame_format(fmt), region) -> lvk_hip_egress_obs
// (Y800: lvk_hip_fsr_easu_gray).  Routes, chosen by the host (obs::fsr_route of the format and lvk_hip_fsr_obs_path):
//   I420 / I40A / NV12              the body of lvk_hip_fsr_yuv420 (lvk_fsr_420, fsr_420.hip)
//   4:2:2, 4:4:4, AYUV              k_fsr_planes (fsr_planes.hpp) into the format's sink (obs_sinks.hpp), which does the egress.  Staged: ONE launch, the
//                                   stage filled from the planes through FsrSrc, which forms the packed pixels the ingest would write.  Direct:
//                                   lvk_launch_ingest_obs into a frame from the context's pool (back in the pool inside the call), the taps read it.
//   BGR3, RGBA / BGRA / BGRX        lvk_hip_fsr_easu on three-byte pixels from the input plane to the output plane: BGR3 at its pitches, the 4-byte formats
//                                   on DirectIngest's views of pitch 3 * cols in and 3 * out_cols out
//   Y800                            lvk_hip_fsr_easu_gray from plane to plane
// No route makes an output-sized packed frame and none ends in lvk_hip_egress_obs.
#include "lvk_hip_internal.hpp"
#include "fsr_planes.hpp"
#include "obs_sinks.hpp"

namespace {

// The planes of a 4:2:2 or 4:4:4 frame as the source of packed pixels 0x00VVUUYY, one pixel at (sx, sy) inside the frame.
// CHROMA 422: LAYOUT 0 planes Y, U, V (I422 / I42A), 1 YUY2, 2 YVYU, 3 UYVY -- the layouts of Sink422; the chroma is up2x's closed form
// (far + 3 near + 2) >> 2 with the edge sample replicated (k_ingest_422, ingest.hip).  CHROMA 444: LAYOUT 0 planes Y, U, V (I444 / YUVA), 1 AYUV -- those
// of Sink444; the bytes themselves.
template <int CHROMA, int LAYOUT>
struct FsrSrc
{
    const uint8_t* p0; int s0; const uint8_t* p1; int s1; const uint8_t* p2; int s2;
    int cc;                                // chroma columns of a 4:2:2 row

    __device__ __forceinline__ uint32_t px(int sx, int sy) const
    {
        const uint8_t* r0 = p0 + (size_t)sy * s0;
        if constexpr (CHROMA == 444 && LAYOUT == 0)
            return (uint32_t)r0[sx] | ((uint32_t)p1[(size_t)sy * s1 + sx] << 8) | ((uint32_t)p2[(size_t)sy * s2 + sx] << 16);
        else if constexpr (CHROMA == 444)
        {
            const uint8_t* q = r0 + 4 * (size_t)sx;                            // A Y U V: the plane may start at any byte
            return (uint32_t)q[1] | ((uint32_t)q[2] << 8) | ((uint32_t)q[3] << 16);
        }
        else
        {
            const int c = sx >> 1, f = min(max((sx & 1) ? c + 1 : c - 1, 0), cc - 1);
            uint32_t y, un, uf, vn, vf;
            if constexpr (LAYOUT == 0)
            {
                const uint8_t* r1 = p1 + (size_t)sy * s1;
                const uint8_t* r2 = p2 + (size_t)sy * s2;
                y = r0[sx]; un = r1[c]; uf = r1[f]; vn = r2[c]; vf = r2[f];
            }
            else
            {
                // a pixel pair is four bytes: Y U Y V (YUY2), Y V Y U (YVYU), U Y V Y (UYVY)
                constexpr int YB = LAYOUT == 3 ? 1 : 0, UB = LAYOUT == 1 ? 1 : LAYOUT == 2 ? 3 : 0, VB = LAYOUT == 1 ? 3 : LAYOUT == 2 ? 1 : 2;
                y = r0[2 * sx + YB]; un = r0[4 * c + UB]; uf = r0[4 * f + UB]; vn = r0[4 * c + VB]; vf = r0[4 * f + VB];
            }
            return y | (((uf + 3 * un + 2) >> 2) << 8) | (((vf + 3 * vn + 2) >> 2) << 16);
        }
    }
};

// the plane source that reads what `Sink` writes
template <class Sink> struct FsrSrcOf;
template <int L> struct FsrSrcOf<Sink422<L>> { using type = FsrSrc<422, L>; };
template <int L> struct FsrSrcOf<Sink444<L>> { using type = FsrSrc<444, L>; };

// the out-tile through a sink: thread t of the block hands the four pixels 4 (t & 15) .. of tile row t >> 4 to it
template <class Sink>
struct SinkOut
{
    Sink sink;
    __device__ __forceinline__ void store_tile(const float* tile, int x0, int y0, int out_rows, int out_cols, int tid) const
    {
        const int r = tid >> 4, x = x0 + PXT * (tid & 15), y = y0 + r;
        if (x >= out_cols || y >= out_rows) return;
        uint32_t px[PXT];
#pragma unroll
        for (int p = 0; p < PXT; p++) px[p] = as_u(tile[r * kTileW + PXT * (tid & 15) + p]);
        store_row(sink, x, y, min(PXT, out_cols - x), px);
    }
};

static_assert(PXT == 4 && kTileW % PXT == 0 && kTileW / PXT * kTileH == 256, "one thread per group of four pixels of the tile");

} // namespace

extern "C" int lvk_hip_fsr_obs(lvk_hip_ctx* ctx, int video_format,
                               const void* const d_planes[3], const int steps[3], int rows, int cols, const int region_xywh[4],
                               void* const o_planes[3], const int o_steps[3], int out_rows, int out_cols)
{
    LVK_HIP_ENTRY(ctx);
    const char* name = "lvk_hip_fsr_obs";
    const int vf = video_format;
    LVK_HIP_REQUIRE(ctx, d_planes != nullptr && steps != nullptr && region_xywh != nullptr && o_planes != nullptr && o_steps != nullptr);
    if (fsr_route(vf, true) == FsrRoute::None)
        return ctx->fail(LVK_HIP_ERR_ARG, std::string(name) + ": video format " + std::to_string(vf) + " is not one FrameIngest::Select knows");
    if (fsr_route(vf, true) == FsrRoute::Planes420)
        return lvk_fsr_420(ctx, name, plane_set_420(vf, d_planes, steps, rows, cols), region_xywh, plane_set_420(vf, o_planes, o_steps, out_rows, out_cols));

    // ---- everything that can refuse the call, before anything is enqueued
    int rc = lvk_ingest_obs_check(ctx, vf, d_planes, steps, rows, cols);          // the planes in use, their pitches, the parity of the size, the format
    if (rc != LVK_HIP_OK) return rc;
    LVK_HIP_REQUIRE(ctx, obs_size_ok(vf, rows, cols) && obs_size_ok(vf, out_rows, out_cols));
    if (!fsr_region_ok(region_xywh, rows, cols))
        return ctx->fail(LVK_HIP_ERR_ARG, std::string(name) + ": the region must be a non-empty rectangle inside the frame");
    // out of place: the taps and the chroma up-sampling read their neighbours, and the input planes are never written
    const Spans in = obs_spans(vf, d_planes, steps, rows, cols);
    if ((rc = obs_outputs_ok(ctx, name, vf, o_planes, o_steps, out_rows, out_cols, in.s, in.n)) != LVK_HIP_OK) return rc;

    const bool staged = lvk_hip_fsr_obs_path(region_xywh[2], region_xywh[3], out_rows, out_cols) == 0;
    const FsrRoute route = fsr_route(vf, staged);
    if (route == FsrRoute::Gray)
        return lvk_hip_fsr_easu_gray(ctx, d_planes[0], steps[0], rows, cols, region_xywh, o_planes[0], o_steps[0], out_rows, out_cols);
    if (route == FsrRoute::Bgr)
    {
        // BGR3 and the DirectIngest formats ARE packed three-byte frames -- BGR3 at its own pitch, RGBA / BGRA / BGRX the first rows * cols * 3 bytes of the
        // tight plane, a frame of pitch 3 * cols at its own size (lvk_ingest_obs_check) --, so ingest and egress are copies and the kernel runs from plane
        // to plane
        const bool tight = is_direct4(vf);
        return lvk_hip_fsr_easu(ctx, d_planes[0], tight ? 3 * cols : steps[0], rows, cols, lvk_hip_obs_frame_format(vf), region_xywh,
                                o_planes[0], tight ? 3 * out_cols : o_steps[0], out_rows, out_cols);
    }

    const FsrGeo geo = fsr_geo(rows, cols, region_xywh, out_rows, out_cols);
    if (route == FsrRoute::FusedPlanes)
        return with_obs_sink(ctx, name, vf, out_rows, out_cols, o_planes, o_steps, [&](const auto& sink) {
            using Sink = std::decay_t<decltype(sink)>;
            using Src = typename FsrSrcOf<Sink>::type;
            const Src src{(const uint8_t*)d_planes[0], steps[0], (const uint8_t*)d_planes[1], steps[1], (const uint8_t*)d_planes[2], steps[2], cols / 2};
            return launch_fsr_planes<Src, SinkOut<Sink>, true>(ctx, src, SinkOut<Sink>{sink}, geo);
        });

    // The frame between the two launches comes from the context's pool and goes back to it once the second is enqueued: whoever is handed it next
    // enqueues behind that kernel on this context's stream (lvk_hip.h, lvk_hip_free), and the steady state allocates nothing.
    void* d_frame = nullptr;
    const int step = fsr_packed_step(cols);
    if ((rc = lvk_hip_malloc(ctx, (size_t)step * rows, &d_frame)) != LVK_HIP_OK) return rc;
    if ((rc = lvk_launch_ingest_obs(ctx, ctx->stream, vf, d_planes, steps, rows, cols, d_frame, step)) == LVK_HIP_OK)
        rc = with_obs_sink(ctx, name, vf, out_rows, out_cols, o_planes, o_steps, [&](const auto& sink) {
            using Sink = std::decay_t<decltype(sink)>;
            return launch_fsr_planes<PackedYuv, SinkOut<Sink>, false>(ctx, PackedYuv{(const uint8_t*)d_frame, step}, SinkOut<Sink>{sink}, geo);
        });
    (void)lvk_hip_free(ctx, d_frame);
    return rc;
}
