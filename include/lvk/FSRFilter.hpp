// lvk::FSRFilter of the C++ facade: the OBS plugin's FSR filter (Modules/OBS-Plugin/Sources/Scaling/FSRFilter.cpp, Effects/FSREffect.cpp: the
// FidelityFX FSR 1 EASU pass; the plugin leaves sharpening to the CAS filter) over lvk_hip_fsr_geometry and lvk_hip_fsr_easu of lvk_hip.h.
// The plugin runs it as an OBS graphics effect; here it is a VideoFilter, so it chains in CompositeFilter (e.g. ConversionFilter to BGRA,
// FSRFilter, CASFilter) and takes BGR / RGB / YUV and BGRA / RGBA frames, and GRAY frames of one channel (lvk_hip_fsr_easu_gray: channel 0 of the
// pass on (g, g, g)).  The output size follows the current frame.  apply(VideoFrame420, VideoFrame420) takes the plugin's I420 / NV12
// planes in one call (lvk_hip_fsr_yuv420, out of place), apply(VideoFrameOBS, VideoFrameOBS) the planes of every OBS video format (lvk_hip_fsr_obs,
// DESIGN.md section 33).
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

    // The plugin's I420 / NV12 planes in one call (lvk_hip_fsr_yuv420), byte for byte upload_obs_frame -> apply(frame, frame) -> download_ocl_frame
    // without the packed frames between them.  Out of place: `output` is created at the output size of the settings in the input's layout and context.  A
    // frame the geometry skips goes through unchanged: `output` then shares the input's block.  4:2:0 takes even output sizes only.
    using VideoFilter::apply;
    void apply(const VideoFrame420& input, VideoFrame420& output, const bool profile = false)
    {
        LVK_HIP_ASSERT(!input.empty());
        LVK_HIP_ASSERT(&input != &output);
        if (!m_Ctx) m_Ctx = input.context();
        int region[4] = {0, 0, 0, 0}, size[2] = {0, 0};
        if (skips(input.rows, input.cols, region, size)) { output = input; return; }
        if (!size_fits(size, 2, 2, input.nv12 ? "NV12" : "I420")) return;
        sync_gpu(profile); frame_timer().start();
        output.create({size[1], size[0]}, input.nv12, input.context());
        LVK_HIP_ASSERT(output.y() != input.y());
        output.timestamp = input.timestamp;
        run(input.context(), [&] {
            m_Ctx->check(lvk_hip_fsr_yuv420(m_Ctx->get(), input.y(), input.y_step(), input.u(), input.uv_step(), input.v(), input.uv_step(),
                                            input.rows, input.cols, region,
                                            output.y(), output.y_step(), output.u(), output.uv_step(), output.v(), output.uv_step(),
                                            output.rows, output.cols, input.nv12 ? 1 : 0),
                         "FSRFilter::apply(4:2:0)");
        });
        sync_gpu(profile); frame_timer().stop();
    }

    // A frame of ANY OBS video format in one call (lvk_hip_fsr_obs), byte for byte FrameIngest::to_ocl -> apply(frame, frame) ->
    // FrameIngest::to_obs without the packed frames between them.  Out of place: `output` is created at the output size of the settings in the input's
    // format and context (bytes to_obs leaves alone -- the last quarter of an RGBA / BGRA / BGRX plane -- are whatever the fresh block held); the input
    // planes are not written.  A frame the geometry skips goes through unchanged: `output` then shares the input's block.  The 4:2:2 formats take even
    // output widths only, the 4:2:0 formats even output sizes.
    void apply(const VideoFrameOBS& input, VideoFrameOBS& output, const bool profile = false)
    {
        LVK_HIP_ASSERT(!input.empty());
        LVK_HIP_ASSERT(&input != &output);
        if (!m_Ctx) m_Ctx = input.context();
        int region[4] = {0, 0, 0, 0}, size[2] = {0, 0};
        if (skips(input.rows, input.cols, region, size)) { output = input; return; }
        const int f = input.format;
        const bool f420 = f == LVK_VIDEO_FORMAT_I420 || f == LVK_VIDEO_FORMAT_I40A || f == LVK_VIDEO_FORMAT_NV12;
        const bool f422 = f == LVK_VIDEO_FORMAT_I422 || f == LVK_VIDEO_FORMAT_I42A || f == LVK_VIDEO_FORMAT_YUY2 || f == LVK_VIDEO_FORMAT_YVYU
                          || f == LVK_VIDEO_FORMAT_UYVY;
        if (!size_fits(size, f420 ? 2 : 1, f420 || f422 ? 2 : 1, ("video format " + std::to_string(f)).c_str())) return;
        sync_gpu(profile); frame_timer().start();
        output.create({size[1], size[0]}, input.format, input.context());
        LVK_HIP_ASSERT(output.data[0] != input.data[0]);
        output.timestamp = input.timestamp;
        run(input.context(), [&] {
            m_Ctx->check(lvk_hip_fsr_obs(m_Ctx->get(), input.format, reinterpret_cast<const void* const*>(input.data), input.linesize, input.rows, input.cols,
                                         region, reinterpret_cast<void* const*>(output.data), output.linesize, output.rows, output.cols),
                         "FSRFilter::apply(OBS)");
        });
        sync_gpu(profile); frame_timer().stop();
    }

private:
    static bool in_crop_range(int c) { return c >= 0 && c <= 4096; }

    // lvk_hip_fsr_geometry with the filter's settings for a rows x cols frame: the region, the output (rows, cols); true when FSRFilter skips the frame
    bool skips(int rows, int cols, int region[4], int size[2]) const
    {
        const int crop[4] = {m_Settings.crop_left, m_Settings.crop_top, m_Settings.crop_right, m_Settings.crop_bottom};
        int skip = 0;
        const int rc = lvk_hip_fsr_geometry(rows, cols, m_Settings.output_size.height, m_Settings.output_size.width, m_Settings.size_multiplier,
                                            m_Settings.maintain_aspect_ratio ? 1 : 0, crop, region, size, &skip);
        LVK_HIP_ASSERT(rc == LVK_HIP_OK);
        return rc != LVK_HIP_OK || skip != 0;
    }

    // the parity a chroma-subsampled format asks of the output (rows, cols); a failed assertion names the size and the format
    static bool size_fits(const int size[2], int row_multiple, int col_multiple, const char* format)
    {
        if (size[0] % row_multiple == 0 && size[1] % col_multiple == 0) return true;
        lvk::context::assert_handler("FSRFilter.hpp", "apply", "the output size " + std::to_string(size[1]) + " x " + std::to_string(size[0]) + " has the parity "
                                                                + format + " takes");
        return false;
    }

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
