// lvk::ScalingFilter::apply(VideoFrameOBS, VideoFrameOBS) of the C++ facade (include/lvk/LiveVisionKit.hpp): the planes of any OBS video format through
// the scaling filter in one call (lvk_hip_scale_obs).
//
// scaling_obs_facade <video format number> <rows> <cols> <out rows> <out cols> <sharpness> <in.bin> <out.bin>
//   in.bin / out.bin: the planes of the format one after the other, tightly packed.  The output block is filled with 0x5A before the first call, so that
//   bytes the egress leaves alone come back as that.  Applies twice -- into the prepared output and again into it --, checks size, format, timestamp,
//   context and that the input planes are untouched, then the filter's assertions.
#include <lvk/LiveVisionKit.hpp>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "facade_util.hpp"

int main(int argc, char** argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: see the head of scaling_obs_facade.cpp\n"); return 2; }
    const int format = std::atoi(argv[1]);
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), orows = std::atoi(argv[4]), ocols = std::atoi(argv[5]);
    const float sharpness = (float)std::atof(argv[6]);
    const bool yuv = lvk_hip_obs_frame_format(format) == LVK_FORMAT_YUV;

    lvk::VideoFrameOBS input, output;
    input.create({cols, rows}, format);
    std::vector<uint8_t> host(input.bytes()), back(host.size());
    if (!read_file(argv[7], host)) return 2;
    input.upload(host.data(), rows, cols, format, 41);
    output.create({ocols, orows}, format, input.context());
    std::vector<uint8_t> first(output.bytes(), 0x5A), second(first.size());
    output.upload(first.data(), orows, ocols, format, 0, input.context());
    const uint8_t* kept = output.data[0];

    lvk::ScalingFilterSettings settings;
    settings.output_size = cv::Size(ocols, orows); settings.sharpness = sharpness; settings.yuv_input = yuv;
    lvk::ScalingFilter filter(settings);
    filter.apply(input, output, true);
    if (output.empty() || output.rows != orows || output.cols != ocols || output.format != format || output.timestamp != 41) return 1;
    if (output.data[0] != kept || output.data[0] == input.data[0] || output.context() != input.context()) return 1;     // the output of the right size is written, not replaced
    output.download(first.data());
    input.timestamp = 42;
    filter.apply(input, output);
    if (output.data[0] != kept || output.timestamp != 42) return 1;
    output.download(second.data());
    if (second != first) return 1;
    input.download(back.data());
    if (back != host) return 1;                               // out of place: the input planes are as they were
    if (!(filter.timings().average().seconds() > 0.0)) return 1;
    if (!write_file(argv[8], first)) return 2;

    // refused like the reference's asserts: the wrong kind of filter for the frame, a smaller output size, the format's parity, the input as its own output
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0, expected = 0;
    lvk::ScalingFilterSettings s = filter.settings();
    const auto refuses = [&](const lvk::ScalingFilterSettings& bad) {
        lvk::ScalingFilter f(bad);
        lvk::VideoFrameOBS out;
        try { f.apply(input, out); } catch (const std::runtime_error&) { return out.empty() ? 1 : 0; }
        return 0;
    };
    if (format != LVK_VIDEO_FORMAT_Y800) { s.yuv_input = !yuv; refused += refuses(s); s.yuv_input = yuv; expected++; }
    if (cols > 2) { s.output_size = cv::Size(cols - 2, orows); refused += refuses(s); expected++; }
    if (rows > 2) { s.output_size = cv::Size(ocols, rows - 2); refused += refuses(s); expected++; }
    const bool f420 = format == LVK_VIDEO_FORMAT_I420 || format == LVK_VIDEO_FORMAT_I40A || format == LVK_VIDEO_FORMAT_NV12;
    const bool f422 = format == LVK_VIDEO_FORMAT_I422 || format == LVK_VIDEO_FORMAT_I42A || format == LVK_VIDEO_FORMAT_YUY2 || format == LVK_VIDEO_FORMAT_YVYU
                   || format == LVK_VIDEO_FORMAT_UYVY;
    if (f420 || f422) { s.output_size = cv::Size(ocols + 1, orows); refused += refuses(s); expected++; }
    if (f420) { s.output_size = cv::Size(ocols, orows + 1); refused += refuses(s); expected++; }
    try { filter.apply(input, input); } catch (const std::runtime_error&) { refused++; }
    expected++;
    {
        lvk::VideoFrameOBS none, out;
        try { filter.apply(none, out); } catch (const std::runtime_error&) { refused += out.empty() ? 1 : 0; }
        expected++;
    }
    input.download(back.data());
    if (refused != expected || back != host) { std::fprintf(stderr, "%d of %d refused\n", refused, expected); return 1; }
    std::printf("scale obs ok: %d %dx%d -> %dx%d\n", format, cols, rows, output.cols, output.rows);
    return 0;
}
