// lvk::draw_points / draw_rect / draw_text and StabilizationFilter::draw_hud of the C++ facade (include/lvk/Drawing.hpp) called the way the
// plugin's test modes call them (Modules/OBS-Plugin/Sources/Stabilisation/VSFilter.cpp:368-383).
//
// drawing_facade defaults <rows> <cols> <frame.bin> <out.bin>
//   four frames into out.bin, each drawn on a fresh upload of frame.bin with DEFAULT arguments: draw_points (Point2f), draw_rect (Rect),
//   draw_text (Point), and draw_rect (Rect2f) + draw_text (Point2f) whose coordinates go through cvRound.
// drawing_facade hud <format> <rows> <cols> <n frames> <frame time ms> <deviation ms> <clip.bin> <out.bin>
//   n frames through a StabilizationFilter; the last frame it emits is written to out.bin as it came out and again after draw_hud.
//   Prints the stable region.
// drawing_facade refuse
//   draw_points with point_size 0, draw_rect with thickness 0 and draw_text with thickness 0 reach the assert handler; col::rgb2yuv.  No device.
#include <lvk/LiveVisionKit.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "facade_util.hpp"

static const cv::Scalar kColour(7, 200, 99);

static int run_defaults(char** argv)
{
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    std::vector<uint8_t> host((size_t)rows * cols * 3), back(host.size()), all;
    if (!read_file(argv[4], host)) return 2;
    lvk::Frame frame;
    auto fresh = [&] { frame.upload(host.data(), rows, cols, lvk::VideoFrame::BGR, 1); };
    auto keep = [&] { frame.download(back.data()); all.insert(all.end(), back.begin(), back.end()); };

    fresh();
    const std::vector<cv::Point2f> points = {{10.5f, 20.25f}, {0.0f, 0.0f}, {(float)cols, (float)rows}, {100.5f, 50.5f}, {-30.0f, 7.0f}};
    lvk::draw_points(frame, points, kColour);
    keep();
    fresh();
    lvk::draw_rect(frame, cv::Rect(30, 20, 100, 60), kColour);
    keep();
    fresh();
    lvk::draw_text(frame, "LVK 0.12ms {~}", cv::Point(12, 60), kColour);
    keep();
    fresh();
    lvk::draw_rect(frame, cv::Rect2f(30.5f, 21.5f, 100.4f, 59.6f), kColour);          // cvRound: (30, 22, 100, 60)
    lvk::draw_text(frame, "Rect2f", cv::Point2f(40.6f, 70.5f), kColour);              // (41, 70)
    lvk::draw_rect(frame, cv::Rect(5, 5, 0, 9), kColour);                             // empty: cv::rectangle draws nothing
    lvk::draw_points(frame, std::vector<cv::Point>{}, kColour);
    keep();
    if (!write_file(argv[5], all)) return 2;
    std::printf("defaults ok: 4 frames\n");
    return 0;
}

static int run_hud(char** argv)
{
    const int fmt = std::atoi(argv[2]), rows = std::atoi(argv[3]), cols = std::atoi(argv[4]), n = std::atoi(argv[5]);
    const double frame_time_ms = std::atof(argv[6]), deviation_ms = std::atof(argv[7]);
    const size_t frame_bytes = (size_t)rows * cols * 3;
    std::vector<uint8_t> clip(frame_bytes * n), back(frame_bytes), all;
    if (!read_file(argv[8], clip)) return 2;
    lvk::StabilizationFilterSettings settings;
    settings.predictive_samples = 3;
    lvk::StabilizationFilter filter(settings);
    lvk::Frame frame, out, last;
    for (int k = 0; k < n; k++)
    {
        frame.upload(clip.data() + frame_bytes * k, rows, cols, (lvk::VideoFrame::Format)fmt, 100 + k);
        filter.apply(std::move(frame), out);
        if (!out.empty()) last = out;
    }
    if (last.empty() || last.format != (lvk::VideoFrame::Format)fmt || last.rows != rows || last.cols != cols) return 1;
    last.download(back.data());
    all.insert(all.end(), back.begin(), back.end());
    filter.draw_hud(last, frame_time_ms, deviation_ms);
    last.download(back.data());
    all.insert(all.end(), back.begin(), back.end());
    if (!write_file(argv[9], all)) return 2;
    const cv::Rect region = filter.stable_region();
    std::printf("hud ok: region %d %d %d %d\n", region.x, region.y, region.width, region.height);
    return 0;
}

static int run_refuse()
{
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0;
    lvk::Frame none;
    try { lvk::draw_points(none, std::vector<cv::Point2f>{{1.0f, 1.0f}}, kColour, 0); } catch (const std::runtime_error&) { refused++; }
    try { lvk::draw_points(none, std::vector<cv::Point2f>{{1.0f, 1.0f}}, kColour, 3, {-1.0f, 1.0f}); } catch (const std::runtime_error&) { refused++; }
    try { lvk::draw_rect(none, cv::Rect(0, 0, 4, 4), kColour, 0); } catch (const std::runtime_error&) { refused++; }
    try { lvk::draw_text(none, "a", cv::Point(0, 8), kColour, 1.5, 0); } catch (const std::runtime_error&) { refused++; }
    try { lvk::draw_text(none, "a", cv::Point(0, 8), kColour); } catch (const std::runtime_error&) { refused++; }          // an empty frame
    const cv::Scalar m = lvk::col::rgb2yuv({255, 0, 255});
    if (std::fabs(m[0] - 106.525) > 1e-9 || std::fabs(m[1] - 202.205) > 1e-9 || std::fabs(m[2] - 221.84) > 1e-9) return 1;
    std::printf("refuse ok: %d refused\n", refused);
    return refused == 5 ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc == 6 && std::string(argv[1]) == "defaults") return run_defaults(argv);
    if (argc == 10 && std::string(argv[1]) == "hud") return run_hud(argv);
    if (argc == 2 && std::string(argv[1]) == "refuse") return run_refuse();
    std::fprintf(stderr, "usage: see the head of drawing_facade.cpp\n");
    return 2;
}
