// lvk::LCFilter of the C++ facade: the OBS plugin's lens-correction filter (Modules/OBS-Plugin/Sources/Enhancement/LCFilter.cpp:99-192) over the
// lvk_hip_lens_* object of lvk_hip.h.  The plugin runs it on OBS frames; here it is a VideoFilter, so it chains in
// CompositeFilter (correct the lens, then stabilize) and takes the frames FrameIngest::upload_obs_frame makes -- BGR / RGB / YUV, BGRA / RGBA and
// GRAY -- and, through apply(VideoFrame420, VideoFrame420), the I420 / NV12 planes of the asynchronous path in one call; through
// apply(VideoFrameOBS, VideoFrameOBS) the planes of every OBS video format.
// Included by LiveVisionKit.hpp.
#pragma once

#include <optional>

#include "LiveVisionKit.hpp"

namespace lvk {

struct LCFilterSettings
{
    std::optional<CameraParameters> profile;     // none selected: frames pass through (LCFilter.cpp:102, m_ProfileSelected)
    bool test_mode = false;                      // the 32 x 32 magenta grid, drawn ahead of the warp (LCFilter.cpp:179-183)
};

class LCFilter final : public detail::ContextFilter, public Configurable<LCFilterSettings>
{
public:
    explicit LCFilter(const LCFilterSettings& settings = {}) : ContextFilter("Lens Correction Filter") { configure(settings); }
    ~LCFilter() override
    {
        if (!m_Handle) return;
        hip::ContextLock lock(m_Ctx->mutex());
        lvk_hip_lens_destroy(m_Handle);
    }
    LCFilter(const LCFilter&) = delete;
    LCFilter& operator=(const LCFilter&) = delete;

    void configure(const LCFilterSettings& settings) override                    // LCFilter.cpp:99-129
    {
        LVK_HIP_ASSERT(!settings.profile || (settings.profile->fx != 0.0 && settings.profile->fy != 0.0));
        m_Settings = settings;
        if (m_Handle)
        {
            lvk_camera_params p;
            hip::ContextLock lock(m_Ctx->mutex());
            m_Ctx->check(lvk_hip_lens_configure(m_Handle, to_c(settings, p), settings.test_mode ? 1 : 0), "LCFilter::configure");
        }
    }

    // The OBS asynchronous path in one call: I420 / NV12 planes in, planes out (lvk_hip_lens_apply_yuv420), byte for byte upload_obs_frame ->
    // apply(frame, frame) -> download_ocl_frame without the packed destination frame.  Out of place: `output` is created at the input's size, layout
    // and context; the input planes are not written, in test mode either.
    using VideoFilter::apply;
    void apply(const VideoFrame420& input, VideoFrame420& output, const bool profile = false)
    {
        LVK_HIP_ASSERT(!input.empty());
        LVK_HIP_ASSERT(&input != &output);
        ensure(input.context());
        sync_gpu(profile); frame_timer().start();
        output.create({input.cols, input.rows}, input.nv12, input.context());
        LVK_HIP_ASSERT(output.y() != input.y());
        output.timestamp = input.timestamp;
        run(input.context(), [&] {
            m_Ctx->check(lvk_hip_lens_apply_yuv420(m_Handle, input.y(), input.y_step(), input.u(), input.uv_step(), input.v(), input.uv_step(),
                                                   output.y(), output.y_step(), output.u(), output.uv_step(), output.v(), output.uv_step(),
                                                   input.rows, input.cols, input.nv12 ? 1 : 0),
                         "LCFilter::apply(4:2:0)");
        });
        sync_gpu(profile); frame_timer().stop();
    }

    // The plugin's LCFilter::filter(OBSFrame&) for a frame of ANY OBS video format in one call (lvk_hip_lens_apply_obs): byte for byte
    // FrameIngest::to_ocl -> filter -> FrameIngest::to_obs.  Out of place: `output` is created at the input's size, format and context (bytes to_obs
    // leaves alone -- the last quarter of an RGBA / BGRA / BGRX plane -- are whatever the fresh block held); the input planes are not written.
    // A Y800 frame is refused in test mode.
    void apply(const VideoFrameOBS& input, VideoFrameOBS& output, const bool profile = false)
    {
        LVK_HIP_ASSERT(!input.empty());
        LVK_HIP_ASSERT(&input != &output);
        LVK_HIP_ASSERT(input.format != LVK_VIDEO_FORMAT_Y800 || !m_Settings.test_mode);
        ensure(input.context());
        sync_gpu(profile); frame_timer().start();
        output.create({input.cols, input.rows}, input.format, input.context());
        LVK_HIP_ASSERT(output.data[0] != input.data[0]);
        output.timestamp = input.timestamp;
        run(input.context(), [&] {
            m_Ctx->check(lvk_hip_lens_apply_obs(m_Handle, input.format, reinterpret_cast<const void* const*>(input.data), input.linesize,
                                                reinterpret_cast<void* const*>(output.data), output.linesize, input.rows, input.cols),
                         "LCFilter::apply(OBS)");
        });
        sync_gpu(profile); frame_timer().stop();
    }

    // the valid-pixel region of a frame of `size` under the profile (cv::getOptimalNewCameraMatrix's ROI); the whole frame without one
    cv::Rect view_region(const cv::Size& size)
    {
        LVK_HIP_ASSERT(size.width > 0 && size.height > 0);
        if (!m_Settings.profile) return cv::Rect(0, 0, size.width, size.height);
        ensure(hip::shared_context());                // asked before the first frame: the object lives on this thread's context
        int r[4] = {0, 0, 0, 0};
        m_Ctx->check(lvk_hip_lens_view(m_Handle, size.height, size.width, r), "LCFilter::view_region");
        return cv::Rect(r[0], r[1], r[2], r[3]);
    }

private:
    static const lvk_camera_params* to_c(const LCFilterSettings& s, lvk_camera_params& p)
    {
        if (!s.profile) return nullptr;
        const CameraParameters& c = *s.profile;
        p.fx = c.fx; p.fy = c.fy; p.cx = c.cx; p.cy = c.cy; p.k1 = c.k1; p.k2 = c.k2; p.p1 = c.p1; p.p2 = c.p2; p.k3 = c.k3;
        return &p;
    }

    void ensure(const std::shared_ptr<hip::Context>& ctx)
    {
        if (m_Handle) return;
        m_Ctx = ctx;
        lvk_camera_params p;
        hip::ContextLock lock(m_Ctx->mutex());
        m_Ctx->check(lvk_hip_lens_create(m_Ctx->get(), to_c(m_Settings, p), m_Settings.test_mode ? 1 : 0, &m_Handle), "LCFilter");
    }

    void filter(VideoFrame&& input, VideoFrame& output) override                 // LCFilter.cpp:175-192; out of place, into a fresh frame
    {
        LVK_HIP_ASSERT(!input.empty());
        const int type = input.type();
        LVK_HIP_ASSERT((type == CV_8UC3 && (input.format == VideoFrame::BGR || input.format == VideoFrame::RGB || input.format == VideoFrame::YUV))
                       || (type == CV_8UC1 && input.format == VideoFrame::GRAY)
                       || (type == CV_8UC4 && (input.format == VideoFrame::BGRA || input.format == VideoFrame::RGBA)));
        LVK_HIP_ASSERT(type == CV_8UC3 || !m_Settings.test_mode);              // the grid kernel writes three bytes per pixel
        VideoFrame src = std::move(input);
        ensure(src.context());
        VideoFrame dst(src.timestamp);
        dst.create(src.size(), src.type(), m_Ctx);
        dst.format = src.format;
        run(src, [&] {
            void* s = src.device_ptr(); void* d = dst.device_ptr();
            const int ss = (int)src.step, ds = (int)dst.step, rows = src.rows, cols = src.cols;
            m_Ctx->check(type == CV_8UC1   ? lvk_hip_lens_apply_gray(m_Handle, s, ss, rows, cols, d, ds)
                         : type == CV_8UC4 ? lvk_hip_lens_apply_c4(m_Handle, s, ss, rows, cols, (int)src.format, d, ds)
                                           : lvk_hip_lens_apply(m_Handle, s, ss, rows, cols, (int)src.format, d, ds),
                         "LCFilter::filter");
        });
        output = std::move(dst);
    }

    lvk_hip_lens* m_Handle = nullptr;
};

} // namespace lvk
