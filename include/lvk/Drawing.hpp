// The rest of Functions/Drawing.hpp of the C++ facade: lvk::draw_points, lvk::draw_rect and lvk::draw_text with the reference's parameter
// order and defaults (Drawing.hpp:76-124), col::rgb2yuv (Drawing.tpp:29-36) and StabilizationFilter::draw_hud, the plugin's
// VSFilter::draw_debug_hud (Modules/OBS-Plugin/Sources/Stabilisation/VSFilter.cpp:368-383).  lvk::draw_grid, lvk::draw_crosses and the colour
// constants are in WarpMesh.hpp.  The reference draws rectangles and text with cv::rectangle / cv::putText on a cv::UMat, which maps the frame
// to the host in the middle of a GPU pipeline; here they are kernels (lvk_hip_draw_rect / lvk_hip_draw_text of lvk_hip.h): in place on a packed
// 8UC3 device frame, asynchronous on the frame's context.  Two declared choices: the font is this library's own 5 x 7
// one, not OpenCV's Hershey glyphs, and a band thicker than one pixel has square corners.  Included by LiveVisionKit.hpp.
#pragma once

#include "LiveVisionKit.hpp"

#ifdef LVK_WITH_OPENCV
#include <opencv2/imgproc.hpp>
#endif

namespace lvk {

namespace col {
inline cv::Scalar rgb2yuv(const cv::Scalar& rgb)                               // Drawing.tpp:29-36
{
    return cv::Scalar(0.257 * rgb[0] + 0.504 * rgb[1] + 0.098 * rgb[2] + 16,
                      -0.148 * rgb[0] - 0.291 * rgb[1] + 0.439 * rgb[2] + 128,
                      0.439 * rgb[0] - 0.368 * rgb[1] - 0.071 * rgb[2] + 128);
}
} // namespace col

namespace detail {
inline int cv_round(const double v) { return (int)std::lrint(v); }             // cvRound: half to even
}

template <typename T>
inline void draw_points(VideoFrame& dst, const std::vector<cv::Point_<T>>& points, const cv::Scalar& color, const int32_t point_size = 10,
                        const cv::Size2f& coord_scaling = {1.0f, 1.0f})
{
    LVK_HIP_ASSERT(coord_scaling.width >= 0 && coord_scaling.height >= 0 && point_size >= 1);
    LVK_HIP_ASSERT(!dst.empty() && dst.type() == CV_8UC3);
    if (points.empty()) return;
    std::vector<float> xy(points.size() * 2);
    for (size_t i = 0; i < points.size(); i++) { xy[2 * i] = (float)points[i].x; xy[2 * i + 1] = (float)points[i].y; }
    const uint8_t c[3] = {(uint8_t)color[0], (uint8_t)color[1], (uint8_t)color[2]};
    const auto& ctx = dst.context();
    hip::ContextLock lock(ctx->mutex());
    ctx->check(lvk_hip_draw_points(ctx->get(), dst.device_ptr(), (int)dst.step, dst.rows, dst.cols, xy.data(), (int)points.size(),
                                   coord_scaling.width, coord_scaling.height, c, point_size), "draw_points");
}

// cv::rectangle(dst, rect, color, thickness): nothing is drawn for an empty rectangle; thickness < 0 fills
template <typename T>
inline void draw_rect(VideoFrame& dst, const cv::Rect_<T>& rect, const cv::Scalar& color, const int thickness = 2)
{
    LVK_HIP_ASSERT(thickness != 0);
    LVK_HIP_ASSERT(!dst.empty() && dst.type() == CV_8UC3);
    const int r[4] = {detail::cv_round((double)rect.x), detail::cv_round((double)rect.y), detail::cv_round((double)rect.width),
                      detail::cv_round((double)rect.height)};                  // (cv::Rect_<T> -> cv::Rect saturates through cvRound)
    if (r[2] <= 0 || r[3] <= 0) return;
    const uint8_t c[3] = {(uint8_t)color[0], (uint8_t)color[1], (uint8_t)color[2]};
    const auto& ctx = dst.context();
    hip::ContextLock lock(ctx->mutex());
    ctx->check(lvk_hip_draw_rect(ctx->get(), dst.device_ptr(), (int)dst.step, dst.rows, dst.cols, r, c, thickness), "draw_rect");
}

// cv::putText(dst, text, position, font, font_scale, color, font_thickness) with the device font: `font` is ignored, and every font pixel is a
// block of max(1, cvRound(2 font_scale)) pixels (the default 1.5 gives 3)
template <typename T>
inline void draw_text(VideoFrame& dst, const std::string& text, const cv::Point_<T>& position, const cv::Scalar& color, const double font_scale = 1.5,
                      const int font_thickness = 2, const cv::HersheyFonts font = cv::FONT_HERSHEY_DUPLEX)
{
    (void)font;
    LVK_HIP_ASSERT(font_thickness >= 1);
    LVK_HIP_ASSERT(!dst.empty() && dst.type() == CV_8UC3);
    const uint8_t c[3] = {(uint8_t)color[0], (uint8_t)color[1], (uint8_t)color[2]};
    const auto& ctx = dst.context();
    hip::ContextLock lock(ctx->mutex());
    ctx->check(lvk_hip_draw_text(ctx->get(), dst.device_ptr(), (int)dst.step, dst.rows, dst.cols, text.c_str(), detail::cv_round((double)position.x),
                                 detail::cv_round((double)position.y), c, std::max(1, detail::cv_round(2.0 * font_scale)), font_thickness), "draw_text");
}

inline void StabilizationFilter::draw_hud(VideoFrame& frame, const double frame_time_ms, const double deviation_ms, const double timing_threshold_ms) const
{
    LVK_HIP_ASSERT(frame.has_known_format());
    const cv::Rect crop_region = stable_region();
    char text[64];
    std::snprintf(text, sizeof text, "%.2fms (%.2fms)", frame_time_ms, deviation_ms);
    draw_text(frame, text, crop_region.tl() + cv::Point(5, 40), frame_time_ms < timing_threshold_ms ? col::GREEN[frame.format] : col::RED[frame.format]);
    draw_rect(frame, crop_region, col::MAGENTA[frame.format]);
}

} // namespace lvk
