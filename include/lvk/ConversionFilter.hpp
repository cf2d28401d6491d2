// lvk::ConversionFilter of the C++ facade (Filters/ConversionFilter.hpp / .cpp: a VideoFilter around cv::cvtColor) over lvk_hip_reformat and
// lvk_hip_cvt_code_target of lvk_hip.h.  It takes the codes between the six VideoFrame formats (cv_min.hpp's ColorConversionCodes) and
// converts out of place into a fresh frame on the device.  The output is tagged with the code's destination format (the reference keeps the
// input's tag; the facade's filters dispatch on it -- DESIGN.md section 15).  Included by LiveVisionKit.hpp; chains in CompositeFilter.
#pragma once

#include "LiveVisionKit.hpp"

#include <optional>
#ifdef LVK_WITH_OPENCV
#include <opencv2/imgproc.hpp>
#endif

namespace lvk {

struct ConversionFilterSettings
{
    cv::ColorConversionCodes conversion_code = cv::COLOR_BGR2YUV;
    std::optional<size_t> output_channels;                 // cvtColor's dcn (none: 0, the code's own)
};

class ConversionFilter final : public detail::ContextFilter, public Configurable<ConversionFilterSettings>
{
public:
    explicit ConversionFilter(const ConversionFilterSettings& settings = {}) : ContextFilter("Conversion Filter") { configure(settings); }
    explicit ConversionFilter(const cv::ColorConversionCodes conversion_code)
        : ConversionFilter(ConversionFilterSettings{conversion_code, std::nullopt}) {}
    ConversionFilter(const ConversionFilter&) = delete;
    ConversionFilter& operator=(const ConversionFilter&) = delete;

    // the code must be one of the supported ones and output_channels 0 or its channel count (4 also for YUV2BGR / YUV2RGB); a refused
    // configure keeps the settings it had
    void configure(const ConversionFilterSettings& settings) override
    {
        bool supported = false;
        if (!settings.output_channels || *settings.output_channels <= 4)
            for (int f = LVK_FORMAT_BGR; f <= LVK_FORMAT_GRAY; f++)
                supported = supported || lvk_hip_cvt_code_target((int)settings.conversion_code, f, dcn_of(settings)) >= 0;
        LVK_HIP_ASSERT(supported);
        if (!supported) return;
        m_Settings = settings;
    }

private:
    static int dcn_of(const ConversionFilterSettings& s) { return s.output_channels ? (int)*s.output_channels : 0; }

    void filter(VideoFrame&& input, VideoFrame& output) override                    // ConversionFilter.cpp:46-57
    {
        LVK_HIP_ASSERT(!input.empty());
        LVK_HIP_ASSERT(input.has_known_format() && input.channels() == VideoFrame::channels_of(input.format));
        const int to = lvk_hip_cvt_code_target((int)m_Settings.conversion_code, (int)input.format, dcn_of(m_Settings));
        LVK_HIP_ASSERT(to >= 0);                           // cvtColor would refuse the frame's channel count
        if (to < 0) return;
        VideoFrame src = std::move(input);
        adopt(src);
        VideoFrame dst(src.timestamp);
        dst.create(src.size(), VideoFrame::type_of((VideoFrame::Format)to), m_Ctx);
        dst.format = (VideoFrame::Format)to;
        run(src, [&] {
            m_Ctx->check(lvk_hip_reformat(m_Ctx->get(), src.device_ptr(), (int)src.step, src.rows, src.cols, (int)src.format, dst.device_ptr(),
                                          (int)dst.step, to), "ConversionFilter::filter");
        });
        output = std::move(dst);
    }
};

} // namespace lvk
