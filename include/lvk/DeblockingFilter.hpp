// lvk::DeblockingFilter of the C++ facade (Filters/DeblockingFilter.{hpp,cpp}) over lvk_hip_deblock_* of lvk_hip.h: same names, settings
// and defaults.  apply(frame, frame) deblocks in place, as the OBS plugin's ADB filter calls it (Modules/OBS-Plugin/Sources/Enhancement/
// ADBFilter.cpp:130-136: apply(frame, frame, true), then draw_influence(frame) in test mode); the filter chains in CompositeFilter and takes the
// frames FrameIngest::upload_obs_frame makes.  filter() dispatches on the frame's type: 8UC3 (BGR / RGB / YUV), 8UC1 of format GRAY and 8UC4 of format
// BGRA / RGBA (lvk_hip_deblock_apply_gray / _c4: the reference's calls per channel, alpha included); draw_influence is 8UC3 only, like the reference's,
// whose overlay is an 8UC3 buffer (DeblockingFilter.cpp:120).  apply(VideoFrame420, VideoFrame420) takes the plugin's I420 / NV12 planes in one call
// (lvk_hip_deblock_apply_yuv420, out of place), apply(VideoFrameOBS, VideoFrameOBS) the planes of every OBS video format
// (lvk_hip_deblock_apply_obs).  Included by LiveVisionKit.hpp.
#pragma once

#include "LiveVisionKit.hpp"

namespace lvk {

struct DeblockingFilterSettings                      // Filters/DeblockingFilter.hpp:27-33
{
    uint32_t detection_levels = 3;   // Must be greater than 0
    uint32_t block_size = 16;        // Must be greater than 0
    uint32_t filter_size = 5;        // Must be odd
    float filter_scaling = 4;        // Smaller is stronger (1/x)
};

class DeblockingFilter final : public detail::ContextFilter, public Configurable<DeblockingFilterSettings>
{
public:
    explicit DeblockingFilter(const DeblockingFilterSettings& settings = {}) : ContextFilter("Deblocking Filter") { configure(settings); }
    ~DeblockingFilter() override
    {
        if (!m_Handle) return;
        hip::ContextLock lock(m_Ctx->mutex());
        lvk_hip_deblock_destroy(m_Handle);
    }
    DeblockingFilter(const DeblockingFilter&) = delete;
    DeblockingFilter& operator=(const DeblockingFilter&) = delete;

    void configure(const DeblockingFilterSettings& settings) override           // DeblockingFilter.cpp:35-45
    {
        LVK_HIP_ASSERT(settings.block_size > 0);
        LVK_HIP_ASSERT(settings.filter_size >= 3);
        LVK_HIP_ASSERT(settings.filter_size % 2 == 1);
        LVK_HIP_ASSERT(settings.detection_levels > 0);
        LVK_HIP_ASSERT(settings.filter_scaling > 1.0f);
        m_Settings = settings;
        if (m_Handle)
        {
            const lvk_deblock_settings s = to_c(settings);
            hip::ContextLock lock(m_Ctx->mutex());
            m_Ctx->check(lvk_hip_deblock_configure(m_Handle, &s), "DeblockingFilter::configure");
        }
    }

    // The OBS asynchronous path in one call: I420 / NV12 planes in, planes out (lvk_hip_deblock_apply_yuv420), byte for byte
    // upload_obs_frame -> apply(frame, frame) -> download_ocl_frame without the packed frame between them.  Out of place: `output` is created at the
    // input's size, layout and context; filter_region() and draw_influence (on a packed 8UC3 frame) answer as after the packed apply.
    using VideoFilter::apply;
    void apply(const VideoFrame420& input, VideoFrame420& output, const bool profile = false)
    {
        LVK_HIP_ASSERT(!input.empty());
        LVK_HIP_ASSERT(&input != &output);
        if (!m_Handle)
        {
            m_Ctx = input.context();
            const lvk_deblock_settings s = to_c(m_Settings);
            hip::ContextLock lock(m_Ctx->mutex());
            m_Ctx->check(lvk_hip_deblock_create(m_Ctx->get(), &s, &m_Handle), "DeblockingFilter");
        }
        sync_gpu(profile); frame_timer().start();
        output.create({input.cols, input.rows}, input.nv12, input.context());
        LVK_HIP_ASSERT(output.y() != input.y());
        output.timestamp = input.timestamp;
        run(input.context(), [&] {
            m_Ctx->check(lvk_hip_deblock_apply_yuv420(m_Handle, input.y(), input.y_step(), input.u(), input.uv_step(), input.v(), input.uv_step(),
                                                      output.y(), output.y_step(), output.u(), output.uv_step(), output.v(), output.uv_step(),
                                                      input.nv12 ? 1 : 0, input.rows, input.cols, nullptr),
                         "DeblockingFilter::apply(4:2:0)");
        });
        sync_gpu(profile); frame_timer().stop();
    }

    // A frame of ANY OBS video format in one call (lvk_hip_deblock_apply_obs), byte for byte FrameIngest::to_ocl -> apply(frame, frame) ->
    // FrameIngest::to_obs without the packed frame between them.  Out of place: `output` is created at the input's size, format and context (bytes
    // to_obs leaves alone -- the last quarter of an RGBA / BGRA / BGRX plane -- are whatever the fresh block held); the input planes are not written;
    // filter_region() and draw_influence (on a packed 8UC3 frame) answer as after the packed apply on the ingested frame.
    void apply(const VideoFrameOBS& input, VideoFrameOBS& output, const bool profile = false)
    {
        LVK_HIP_ASSERT(!input.empty());
        LVK_HIP_ASSERT(&input != &output);
        if (!m_Handle)
        {
            m_Ctx = input.context();
            const lvk_deblock_settings s = to_c(m_Settings);
            hip::ContextLock lock(m_Ctx->mutex());
            m_Ctx->check(lvk_hip_deblock_create(m_Ctx->get(), &s, &m_Handle), "DeblockingFilter");
        }
        sync_gpu(profile); frame_timer().start();
        output.create({input.cols, input.rows}, input.format, input.context());
        LVK_HIP_ASSERT(output.data[0] != input.data[0]);
        output.timestamp = input.timestamp;
        run(input.context(), [&] {
            m_Ctx->check(lvk_hip_deblock_apply_obs(m_Handle, input.format, reinterpret_cast<const void* const*>(input.data), input.linesize,
                                                   reinterpret_cast<void* const*>(output.data), output.linesize, input.rows, input.cols, nullptr),
                         "DeblockingFilter::apply(OBS)");
        });
        sync_gpu(profile); frame_timer().stop();
    }

    void draw_influence(VideoFrame& frame) const                                  // DeblockingFilter.cpp:114-131
    {
        LVK_HIP_ASSERT(m_Handle != nullptr && !frame.empty());
        LVK_HIP_ASSERT(frame.type() == CV_8UC3);
        run(frame, [&] {
            m_Ctx->check(lvk_hip_deblock_draw_influence(m_Handle, frame.device_ptr(), (int)frame.step, frame.rows, frame.cols, (int)frame.format),
                         "DeblockingFilter::draw_influence");
        });
    }

    cv::Rect filter_region() const                                                // DeblockingFilter.cpp:135-138
    {
        int r[4] = {0, 0, 0, 0};
        if (m_Handle) lvk_hip_deblock_filter_region(m_Handle, r);
        return cv::Rect(r[0], r[1], r[2], r[3]);
    }

private:
    static lvk_deblock_settings to_c(const DeblockingFilterSettings& s)
    {
        lvk_deblock_settings c;
        c.detection_levels = s.detection_levels; c.block_size = s.block_size; c.filter_size = s.filter_size; c.filter_scaling = s.filter_scaling;
        return c;
    }

    void filter(VideoFrame&& input, VideoFrame& output) override                  // DeblockingFilter.cpp:48-110, in place
    {
        LVK_HIP_ASSERT(!input.empty());
        const int type = input.type();
        LVK_HIP_ASSERT(type == CV_8UC3 || (type == CV_8UC1 && input.format == VideoFrame::GRAY)
                       || (type == CV_8UC4 && (input.format == VideoFrame::BGRA || input.format == VideoFrame::RGBA)));
        VideoFrame frame = std::move(input);
        if (!m_Handle)
        {
            m_Ctx = frame.context();
            const lvk_deblock_settings s = to_c(m_Settings);
            hip::ContextLock lock(m_Ctx->mutex());
            m_Ctx->check(lvk_hip_deblock_create(m_Ctx->get(), &s, &m_Handle), "DeblockingFilter");
        }
        run(frame, [&] {
            void* p = frame.device_ptr();
            const int step = (int)frame.step, rows = frame.rows, cols = frame.cols;
            m_Ctx->check(type == CV_8UC1   ? lvk_hip_deblock_apply_gray(m_Handle, p, step, rows, cols, nullptr)
                         : type == CV_8UC4 ? lvk_hip_deblock_apply_c4(m_Handle, p, step, rows, cols, (int)frame.format, nullptr)
                                           : lvk_hip_deblock_apply(m_Handle, p, step, rows, cols, (int)frame.format, nullptr),
                         "DeblockingFilter::filter");
        });
        output = std::move(frame);
    }

    lvk_hip_deblock* m_Handle = nullptr;
};

} // namespace lvk
