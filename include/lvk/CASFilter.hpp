// lvk::CASFilter of the C++ facade: the OBS plugin's CAS filter (Modules/OBS-Plugin/Sources/Enhancement/CASFilter.cpp, Effects/CASEffect.cpp:
// contrast adaptive sharpening, FidelityFX CasFilter with CAS_SLOW and CAS_BETTER_DIAGONALS) over lvk_hip_cas of lvk_hip.h.  The plugin runs
// it as an OBS graphics effect; here it is a VideoFilter, so it chains in CompositeFilter (deblock, then sharpen) and takes the frames
// FrameIngest::upload_obs_frame makes: BGR / RGB / YUV, BGRA / RGBA frames of 4 channels (VideoFrame::reformat, ConversionFilter) and GRAY
// frames of one channel (lvk_hip_cas_gray: channel 0 of the filter on (g, g, g)).
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
