// lvk::CASFilter of the C++ facade: the OBS plugin's CAS filter (Modules/OBS-Plugin/Sources/Enhancement/CASFilter.cpp, Effects/CASEffect.cpp:
// contrast adaptive sharpening, FidelityFX CasFilter with CAS_SLOW and CAS_BETTER_DIAGONALS) over lvk_hip_cas of lvk_hip.h.  The plugin runs
// it as an OBS graphics effect; here it is a VideoFilter, so it chains in CompositeFilter (deblock, then sharpen) and takes the frames
// FrameIngest::upload_obs_frame makes: BGR / RGB / YUV, BGRA / RGBA frames of 4 channels (VideoFrame::reformat, ConversionFilter) and GRAY
// frames of one channel (lvk_hip_cas_gray: channel 0 of the filter on (g, g, g)).  apply(VideoFrame420, VideoFrame420) takes the plugin's I420 / NV12
// planes in one call (lvk_hip_cas_yuv420, out of place), apply(VideoFrameOBS, VideoFrameOBS) the planes of every OBS video format (lvk_hip_cas_obs).
// Included by LiveVisionKit.hpp.
#pragma once

#include "LiveVisionKit.hpp"

namespace lvk {

struct CASFilterSettings
{
    float sharpness = 0.8f;          // [0, 1] (CASFilter.cpp: PROP_SHARPNESS_DEFAULT; CASEffect.cpp: LVK_ASSERT_01)
};

class CASFilter final : public detail::ContextFilter, public Configurable<CASFilterSettings>
{
public:
    explicit CASFilter(const CASFilterSettings& settings = {}) : ContextFilter("CAS Filter") { configure(settings); }
    CASFilter(const CASFilter&) = delete;
    CASFilter& operator=(const CASFilter&) = delete;

    void configure(const CASFilterSettings& settings) override
    {
        LVK_HIP_ASSERT(settings.sharpness >= 0.0f && settings.sharpness <= 1.0f);
        m_Settings = settings;
    }

    // The plugin's I420 / NV12 planes in one call (lvk_hip_cas_yuv420), byte for byte upload_obs_frame -> apply(frame, frame) -> download_ocl_frame
    // without the packed frames between them.  Out of place: `output` is created at the input's size, layout and context.
    using VideoFilter::apply;
    void apply(const VideoFrame420& input, VideoFrame420& output, const bool profile = false)
    {
        LVK_HIP_ASSERT(!input.empty());
        LVK_HIP_ASSERT(&input != &output);
        if (!m_Ctx) m_Ctx = input.context();
        sync_gpu(profile); frame_timer().start();
        output.create({input.cols, input.rows}, input.nv12, input.context());
        LVK_HIP_ASSERT(output.y() != input.y());
        output.timestamp = input.timestamp;
        run(input.context(), [&] {
            m_Ctx->check(lvk_hip_cas_yuv420(m_Ctx->get(), input.y(), input.y_step(), input.u(), input.uv_step(), input.v(), input.uv_step(),
                                            output.y(), output.y_step(), output.u(), output.uv_step(), output.v(), output.uv_step(),
                                            input.rows, input.cols, input.nv12 ? 1 : 0, m_Settings.sharpness),
                         "CASFilter::apply(4:2:0)");
        });
        sync_gpu(profile); frame_timer().stop();
    }

    // A frame of ANY OBS video format in one call (lvk_hip_cas_obs), byte for byte FrameIngest::to_ocl -> apply(frame, frame) ->
    // FrameIngest::to_obs without the packed frames between them.  Out of place: `output` is created at the input's size, format and context (bytes
    // to_obs leaves alone -- the last quarter of an RGBA / BGRA / BGRX plane -- are whatever the fresh block held); the input planes are not written.
    void apply(const VideoFrameOBS& input, VideoFrameOBS& output, const bool profile = false)
    {
        LVK_HIP_ASSERT(!input.empty());
        LVK_HIP_ASSERT(&input != &output);
        if (!m_Ctx) m_Ctx = input.context();
        sync_gpu(profile); frame_timer().start();
        output.create({input.cols, input.rows}, input.format, input.context());
        LVK_HIP_ASSERT(output.data[0] != input.data[0]);
        output.timestamp = input.timestamp;
        run(input.context(), [&] {
            m_Ctx->check(lvk_hip_cas_obs(m_Ctx->get(), input.format, reinterpret_cast<const void* const*>(input.data), input.linesize,
                                         reinterpret_cast<void* const*>(output.data), output.linesize, input.rows, input.cols, m_Settings.sharpness),
                         "CASFilter::apply(OBS)");
        });
        sync_gpu(profile); frame_timer().stop();
    }

private:
    void filter(VideoFrame&& input, VideoFrame& output) override
    {
        LVK_HIP_ASSERT(!input.empty());
        const bool gray = input.type() == CV_8UC1;
        LVK_HIP_ASSERT(!gray || input.format == VideoFrame::GRAY);
        VideoFrame src = std::move(input);          // CAS reads its neighbours: out of place, into a fresh frame
        adopt(src);
        VideoFrame dst(src.timestamp);
        dst.create(src.size(), src.type(), m_Ctx);
        dst.format = src.format;
        run(src, [&] {
            m_Ctx->check(gray ? lvk_hip_cas_gray(m_Ctx->get(), src.device_ptr(), (int)src.step, src.rows, src.cols, dst.device_ptr(), (int)dst.step,
                                                 m_Settings.sharpness)
                              : lvk_hip_cas(m_Ctx->get(), src.device_ptr(), (int)src.step, src.rows, src.cols, (int)src.format, dst.device_ptr(),
                                            (int)dst.step, m_Settings.sharpness),
                         "CASFilter::filter");
        });
        output = std::move(dst);
    }
};

} // namespace lvk
