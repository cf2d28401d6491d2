// lvk::DeblockingFilter::apply(VideoFrameOBS, VideoFrameOBS) of the C++ facade (include/lvk/DeblockingFilter.hpp): the planes of any OBS video format
// through the deblocking filter in one call (lvk_hip_deblock_apply_obs).
//
// deblocking_obs_facade <video format number> <rows> <cols> <levels> <block> <k> <scaling> <in.bin> <out.bin>
//   in.bin / out.bin: the planes of the format one after the other, tightly packed.  The output block is filled with 0x5A before the first call, so that
//   bytes the egress leaves alone come back as that.  Applies twice -- into the prepared output and again into it --, checks size, format, timestamp,
//   context, the filter region and that the input planes are untouched, then the filter's assertions.
#include <lvk/LiveVisionKit.hpp>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "facade_util.hpp"

static bool same(const cv::Rect& a, const cv::Rect& b) { return a.x == b.x && a.y == b.y && a.width == b.width && a.height == b.height; }

int main(int argc, char** argv)
{
    if (argc != 10) { std::fprintf(stderr, "usage: see the head of deblocking_obs_facade.cpp\n"); return 2; }
    const int format = std::atoi(argv[1]);
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    lvk::DeblockingFilterSettings settings;
    settings.detection_levels = (uint32_t)std::atoi(argv[4]); settings.block_size = (uint32_t)std::atoi(argv[5]);
    settings.filter_size = (uint32_t)std::atoi(argv[6]); settings.filter_scaling = (float)std::atof(argv[7]);

    lvk::VideoFrameOBS input, output;
    input.create({cols, rows}, format);
    std::vector<uint8_t> host(input.bytes()), back(host.size());
    if (!read_file(argv[8], host)) return 2;
    input.upload(host.data(), rows, cols, format, 41);
    output.create({cols, rows}, format, input.context());
    std::vector<uint8_t> first(output.bytes(), 0x5A), second(first.size());
    output.upload(first.data(), rows, cols, format, 0, input.context());
    const uint8_t* kept = output.data[0];

    lvk::DeblockingFilter filter(settings);
    if (!same(filter.filter_region(), cv::Rect(0, 0, 0, 0))) return 1;
    filter.apply(input, output, true);
    if (output.empty() || output.rows != rows || output.cols != cols || output.format != format || output.timestamp != 41) return 1;
    if (output.data[0] != kept || output.data[0] == input.data[0] || output.context() != input.context()) return 1;     // the output of the right size is written, not replaced
    output.download(first.data());
    const cv::Rect region = filter.filter_region();
    const int bs = (int)settings.block_size;
    if (!same(region, cv::Rect(0, 0, cols / bs * bs, rows / bs * bs))) return 1;
    input.timestamp = 42;
    filter.apply(input, output);
    if (output.data[0] != kept || output.timestamp != 42) return 1;
    output.download(second.data());
    if (second != first) return 1;
    input.download(back.data());
    if (back != host) return 1;                               // out of place: the input planes are as they were
    if (!(filter.timings().average().seconds() > 0.0)) return 1;
    if (!write_file(argv[9], first)) return 2;

    // a fresh output is created at the input's size, format and context
    {
        lvk::VideoFrameOBS made;
        filter.apply(input, made);
        if (made.empty() || made.rows != rows || made.cols != cols || made.format != format || made.context() != input.context() || made.timestamp != 42) return 1;
    }

    // refused like the reference's asserts: the input as its own output, an empty input
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0, expected = 0;
    try { filter.apply(input, input); } catch (const std::runtime_error&) { refused++; }
    expected++;
    {
        lvk::VideoFrameOBS none, out;
        try { filter.apply(none, out); } catch (const std::runtime_error&) { refused += out.empty() ? 1 : 0; }
        expected++;
    }
    input.download(back.data());
    if (refused != expected || back != host || !same(filter.filter_region(), region)) { std::fprintf(stderr, "%d of %d refused\n", refused, expected); return 1; }
    std::printf("deblock obs ok: %d %dx%d region %dx%d\n", format, cols, rows, region.width, region.height);
    return 0;
}
