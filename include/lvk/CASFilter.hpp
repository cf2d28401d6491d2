// lvk::CASFilter of the C++ facade: the OBS plugin's CAS filter (Modules/OBS-Plugin/Sources/Enhancement/CASFilter.cpp, Effects/CASEffect.cpp:
// contrast adaptive sharpening, FidelityFX CasFilter with CAS_SLOW and CAS_BETTER_DIAGONALS) over lvk_hip_cas of lvk_hip.h.  The plugin runs
// it as an OBS graphics effect; here it is a VideoFilter, so it chains in CompositeFilter (deblock, then sharpen) and takes the frames
// FrameIngest::upload_obs_frame makes: BGR / RGB / YUV, and BGRA / RGBA frames of 4 channels (VideoFrame::reformat, ConversionFilter).
// Included by LiveVisionKit.hpp.
#pragma once

#include "LiveVisionKit.hpp"

namespace lvk {

struct CASFilterSettings
{
    float sharpness = 0.8f;          // [0, 1] (CASFilter.cpp: PROP_SHARPNESS_DEFAULT; CASEffect.cpp: LVK_ASSERT_01)
};

class CASFilter final : public VideoFilter, public Configurable<CASFilterSettings>
{
public:
    explicit CASFilter(const CASFilterSettings& settings = {}) : VideoFilter("CAS Filter") { configure(settings); }
    CASFilter(const CASFilter&) = delete;
    CASFilter& operator=(const CASFilter&) = delete;

    void configure(const CASFilterSettings& settings) override
    {
        LVK_HIP_ASSERT(settings.sharpness >= 0.0f && settings.sharpness <= 1.0f);
        m_Settings = settings;
    }

private:
    // frames of another context (a chain whose stages run on different streams) are fenced in both directions around the filter's work
    void fence_in(const VideoFrame& frame) const { if (frame.context() && frame.context() != m_Ctx) m_Ctx->wait_for(*frame.context()); }
    void fence_out(const VideoFrame& frame) const { if (frame.context() && frame.context() != m_Ctx) frame.context()->wait_for(*m_Ctx); }

    void filter(VideoFrame&& input, VideoFrame& output) override
    {
        LVK_HIP_ASSERT(!input.empty());
        VideoFrame src = std::move(input);          // CAS reads its neighbours: out of place, into a fresh frame
        if (!m_Ctx) m_Ctx = src.context();
        VideoFrame dst(src.timestamp);
        dst.create(src.size(), src.type(), m_Ctx);
        dst.format = src.format;
        {
            hip::ContextLock lock(m_Ctx->mutex());
            fence_in(src);
            m_Ctx->check(lvk_hip_cas(m_Ctx->get(), src.device_ptr(), (int)src.step, src.rows, src.cols, (int)src.format, dst.device_ptr(),
                                     (int)dst.step, m_Settings.sharpness), "CASFilter::filter");
            fence_out(src);
        }
        output = std::move(dst);
    }
    void sync_gpu(bool trigger) override { if (trigger && m_Ctx) { hip::ContextLock lock(m_Ctx->mutex()); m_Ctx->check(lvk_hip_sync(m_Ctx->get()), "sync_gpu"); } }

    std::shared_ptr<hip::Context> m_Ctx;
};

} // namespace lvk
