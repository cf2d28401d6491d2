// lvk::FSRFilter on the planes of an I420 / NV12 frame, out of place: lvk_hip_fsr_yuv420.  The output planes are, byte for byte,
// those of lvk_hip_ingest_yuv420 -> lvk_hip_fsr_easu(format = YUV, region) -> lvk_hip_egress_yuv420, without the output-sized packed frame.
//
// The kernel is k_fsr_planes (fsr_planes.hpp), four instances: I420 / NV12 planes out, each with
//   staged   Src420 -- the planes themselves, up-sampled into the LDS stage: ONE launch, no packed frame at all
//   direct   PackedYuv -- lvk_launch_ingest_yuv420 into a frame from the context's pool, which goes back to the pool inside the call (whoever is handed
//            it next enqueues behind this kernel on the context's stream), then the taps read that frame
// chosen by lvk_hip_fsr_obs_path: fsr_stage_fits (fsr_core.hpp) against the stage of float4 texels.
#include "lvk_hip_internal.hpp"
#include "fsr_planes.hpp"

using namespace yuv420;

extern "C" int lvk_hip_fsr_obs_path(int rw, int rh, int out_rows, int out_cols)
{
    return fsr_stage_fits(rw, rh, out_rows, out_cols, kStageTexels<float4>);
}

// lvk_hip_fsr_yuv420 behind its entry guard: also the I420 / I40A / NV12 route of lvk_hip_fsr_obs (fsr_obs.hip)
int lvk_fsr_420(lvk_hip_ctx* ctx, const char* name, const PlaneSet& src, const int region_xywh[4], const PlaneSet& dst)
{
    LVK_HIP_REQUIRE(ctx, region_xywh != nullptr);
    LVK_HIP_REQUIRE(ctx, well_formed(src) && well_formed(dst, true) && src.nv12 == dst.nv12);
    if (!fsr_region_ok(region_xywh, src.rows, src.cols))
        return ctx->fail(LVK_HIP_ERR_ARG, std::string(name) + ": the region must be a non-empty rectangle inside the frame");
    // out of place: the taps and the chroma up-sampling read their neighbours
    const Spans src_spans = spans_of(src);
    int rc = require_out_of_place(ctx, name, src_spans.s, src_spans.n, dst);
    if (rc != LVK_HIP_OK) return rc;

    const FsrGeo geo = fsr_geo(src.rows, src.cols, region_xywh, dst.rows, dst.cols);
    const int flags = access_flags(nullptr, dst);
    if (lvk_hip_fsr_obs_path(region_xywh[2], region_xywh[3], dst.rows, dst.cols) == 0)
    {
        if (dst.nv12) return launch_fsr_planes<Src420<true>, Out420<true>, true>(ctx, {src.in(), src.rows / 2, src.cols / 2}, {dst.out(), flags}, geo);
        return launch_fsr_planes<Src420<false>, Out420<false>, true>(ctx, {src.in(), src.rows / 2, src.cols / 2}, {dst.out(), flags}, geo);
    }
    void* d_frame = nullptr;
    const int step = fsr_packed_step(src.cols);
    if ((rc = lvk_hip_malloc(ctx, (size_t)step * src.rows, &d_frame)) != LVK_HIP_OK) return rc;
    const Planes& p = src.p;
    rc = lvk_launch_ingest_yuv420(ctx, ctx->stream, p.y, p.ys, p.u, p.us, p.v, p.vs, src.nv12, src.rows, src.cols, d_frame, step);
    if (rc == LVK_HIP_OK)
        rc = dst.nv12 ? launch_fsr_planes<PackedYuv, Out420<true>, false>(ctx, {(const uint8_t*)d_frame, step}, {dst.out(), flags}, geo)
                      : launch_fsr_planes<PackedYuv, Out420<false>, false>(ctx, {(const uint8_t*)d_frame, step}, {dst.out(), flags}, geo);
    (void)lvk_hip_free(ctx, d_frame);
    return rc;
}

extern "C" int lvk_hip_fsr_yuv420(lvk_hip_ctx* ctx,
                                  const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step, int rows, int cols,
                                  const int region_xywh[4],
                                  void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int out_rows, int out_cols, int nv12)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_fsr_420(ctx, "lvk_hip_fsr_yuv420", plane_set(d_y, y_step, d_u, u_step, d_v, v_step, nv12, rows, cols), region_xywh,
                       plane_set(o_y, oy_step, o_u, ou_step, o_v, ov_step, nv12, out_rows, out_cols));
}
