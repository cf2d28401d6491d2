// lvk::ScalingFilter::apply(VideoFrame420, VideoFrame420) of the C++ facade (include/lvk/LiveVisionKit.hpp): the plugin's I420 / NV12 planes through the
// scaling filter in one call (lvk_hip_scale_yuv420).
//
// scaling_420_facade <nv12> <rows> <cols> <out rows> <out cols> <sharpness> <planes.bin> <out.bin>
//   planes.bin: the tight planes (Y, then U and V, or the interleaved UV plane); out.bin: the output's.  Applies twice -- into an empty output and
//   into the one the first call made --, checks size, layout, timestamp, context and that the input planes are untouched, then the filter's assertions.
#include <lvk/LiveVisionKit.hpp>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "facade_util.hpp"

int main(int argc, char** argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: see the head of scaling_420_facade.cpp\n"); return 2; }
    const bool nv12 = std::atoi(argv[1]) != 0;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), orows = std::atoi(argv[4]), ocols = std::atoi(argv[5]);
    const float sharpness = (float)std::atof(argv[6]);
    std::vector<uint8_t> host((size_t)rows * cols * 3 / 2), back(host.size()), first((size_t)orows * ocols * 3 / 2), second(first.size());
    if (!read_file(argv[7], host)) return 2;

    lvk::ScalingFilter filter(cv::Size(ocols, orows), sharpness);
    lvk::VideoFrame420 input, output;
    input.upload(host.data(), rows, cols, nv12, 41);
    filter.apply(input, output, true);
    if (output.empty() || output.rows != orows || output.cols != ocols || output.nv12 != nv12 || output.timestamp != 41) return 1;
    if (output.y() == input.y() || output.context() != input.context()) return 1;
    output.download(first.data());
    const uint8_t* kept = output.y();
    input.timestamp = 42;
    filter.apply(input, output);                              // the output of the right size is written again, not replaced
    if (output.y() != kept || output.timestamp != 42) return 1;
    output.download(second.data());
    if (second != first) return 1;
    input.download(back.data());
    if (back != host) return 1;                               // out of place: the input planes are as they were
    if (!(filter.timings().average().seconds() > 0.0)) return 1;
    if (!write_file(argv[8], first)) return 2;

    // refused like the reference's asserts: a BGR filter, an odd or smaller output size, the input as its own output
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0;
    lvk::ScalingFilterSettings s = filter.settings();
    const auto refuses = [&](const lvk::ScalingFilterSettings& bad) {
        lvk::ScalingFilter f(bad);
        lvk::VideoFrame420 out;
        try { f.apply(input, out); } catch (const std::runtime_error&) { return out.empty() ? 1 : 0; }
        return 0;
    };
    s.yuv_input = false; refused += refuses(s); s.yuv_input = true;
    s.output_size = cv::Size(ocols + 1, orows); refused += refuses(s);
    s.output_size = cv::Size(ocols, orows + 1); refused += refuses(s);
    s.output_size = cv::Size(cols - 2, orows); refused += refuses(s);
    s.output_size = cv::Size(ocols, rows - 2); refused += refuses(s);
    try { filter.apply(input, input); } catch (const std::runtime_error&) { refused++; }
    input.download(back.data());
    if (refused != 6 || back != host) { std::fprintf(stderr, "%d of 6 refused\n", refused); return 1; }
    std::printf("scale 420 ok: %dx%d -> %dx%d\n", cols, rows, output.cols, output.rows);
    return 0;
}
