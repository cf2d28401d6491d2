// lvk::FSRFilter of the C++ facade: the OBS plugin's FSR filter (Modules/OBS-Plugin/Sources/Scaling/FSRFilter.cpp, Effects/FSREffect.cpp: the
// FidelityFX FSR 1 EASU pass; the plugin leaves sharpening to the CAS filter) over lvk_hip_fsr_geometry and lvk_hip_fsr_easu of lvk_hip.h.
// The plugin runs it as an OBS graphics effect; here it is a VideoFilter, so it chains in CompositeFilter (e.g. ConversionFilter to BGRA,
// FSRFilter, CASFilter) and takes BGR / RGB / YUV and BGRA / RGBA frames, and GRAY frames of one channel (lvk_hip_fsr_easu_gray: channel 0 of the
// pass on (g, g, g)).  The output size follows the current frame.
// Included by LiveVisionKit.hpp.
#pragma once

#include "LiveVisionKit.hpp"

namespace lvk {

struct FSRFilterSettings
{
    cv::Size output_size = {0, 0};           // an explicit output size; (0, 0): the frame's size times size_multiplier
    float size_multiplier = 1.0f;            // FSRFilter.cpp: the "x2" / "x0.5" output patterns
    bool maintain_aspect_ratio = true;       // FSRFilter.cpp: MAINTAIN_ASPECT_DEFAULT
    int crop_left = 0, crop_top = 0, crop_right = 0, crop_bottom = 0;     // [0, 4096] (PROP_CROP_MIN / PROP_CROP_MAX)
};

class FSRFilter final : public detail::ContextFilter, public Configurable<FSRFilterSettings>
{
public:
    explicit FSRFilter(const FSRFilterSettings& settings = {}) : ContextFilter("FSR Filter") { configure(settings); }
    FSRFilter(const FSRFilter&) = delete;
    FSRFilter& operator=(const FSRFilter&) = delete;

    // a refused configure keeps the settings it had
    void configure(const FSRFilterSettings& settings) override
    {
        const bool ok = settings.output_size.width >= 0 && settings.output_size.height >= 0 && settings.size_multiplier > 0.0f
                        && std::isfinite(settings.size_multiplier) && in_crop_range(settings.crop_left) && in_crop_range(settings.crop_top)
                        && in_crop_range(settings.crop_right) && in_crop_range(settings.crop_bottom);
        LVK_HIP_ASSERT(ok);
        if (!ok) return;
        m_Settings = settings;
    }

private:
    static bool in_crop_range(int c) { return c >= 0 && c <= 4096; }

    void filter(VideoFrame&& input, VideoFrame& output) override
    {
        LVK_HIP_ASSERT(!input.empty());
        const bool gray = input.type() == CV_8UC1;
        LVK_HIP_ASSERT(!gray || input.format == VideoFrame::GRAY);
        const int crop[4] = {m_Settings.crop_left, m_Settings.crop_top, m_Settings.crop_right, m_Settings.crop_bottom};
        int region[4] = {0, 0, 0, 0}, size[2] = {0, 0}, skip = 0;
        const int rc = lvk_hip_fsr_geometry(input.rows, input.cols, m_Settings.output_size.height, m_Settings.output_size.width,
                                            m_Settings.size_multiplier, m_Settings.maintain_aspect_ratio ? 1 : 0, crop, region, size, &skip);
        LVK_HIP_ASSERT(rc == LVK_HIP_OK);
        if (skip)                                   // FSREffect::should_skip / is_renderable: the frame goes through unchanged
        {
            if (&input != &output) output = std::move(input);
            return;
        }
        VideoFrame src = std::move(input);
        adopt(src);
        VideoFrame dst(src.timestamp);
        dst.create(cv::Size(size[1], size[0]), src.type(), m_Ctx);
        dst.format = src.format;
        run(src, [&] {
            m_Ctx->check(gray ? lvk_hip_fsr_easu_gray(m_Ctx->get(), src.device_ptr(), (int)src.step, src.rows, src.cols, region, dst.device_ptr(),
                                                      (int)dst.step, dst.rows, dst.cols)
                              : lvk_hip_fsr_easu(m_Ctx->get(), src.device_ptr(), (int)src.step, src.rows, src.cols, (int)src.format, region,
                                                 dst.device_ptr(), (int)dst.step, dst.rows, dst.cols),
                         "FSRFilter::filter");
        });
        output = std::move(dst);
    }
};

} // namespace lvk
