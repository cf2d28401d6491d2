// lvk::DeblockingFilter::apply(VideoFrame420, VideoFrame420) of the C++ facade (include/lvk/DeblockingFilter.hpp): the plugin's I420 / NV12 planes
// through the deblocker in one call (lvk_hip_deblock_apply_yuv420).
//
// deblocking_420_facade <nv12> <rows> <cols> <levels> <block> <k> <scaling> <planes.bin> <out.bin>
//   planes.bin: the tight planes (Y, then U and V, or the interleaved UV plane); out.bin: the output's.  Applies twice -- into an empty output and
//   into the one the first call made --, checks size, layout, timestamp and that the input planes are untouched, prints the filter region.
#include <lvk/LiveVisionKit.hpp>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "facade_util.hpp"

int main(int argc, char** argv)
{
    if (argc != 10) { std::fprintf(stderr, "usage: see the head of deblocking_420_facade.cpp\n"); return 2; }
    const bool nv12 = std::atoi(argv[1]) != 0;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    lvk::DeblockingFilterSettings s;
    s.detection_levels = (uint32_t)std::atoi(argv[4]); s.block_size = (uint32_t)std::atoi(argv[5]);
    s.filter_size = (uint32_t)std::atoi(argv[6]); s.filter_scaling = (float)std::atof(argv[7]);
    std::vector<uint8_t> host((size_t)rows * cols * 3 / 2), back(host.size()), first(host.size());
    if (!read_file(argv[8], host)) return 2;

    lvk::DeblockingFilter filter(s);
    lvk::VideoFrame420 input, output;
    input.upload(host.data(), rows, cols, nv12, 41);
    filter.apply(input, output, true);
    if (output.empty() || output.rows != rows || output.cols != cols || output.nv12 != nv12 || output.timestamp != 41) return 1;
    if (output.y() == input.y() || output.context() != input.context()) return 1;
    output.download(first.data());
    const uint8_t* kept = output.y();
    input.timestamp = 42;
    filter.apply(input, output);                              // the output of the right size is written again, not replaced
    if (output.y() != kept || output.timestamp != 42) return 1;
    output.download(back.data());
    if (back != first) return 1;
    input.download(back.data());
    if (back != host) return 1;                               // out of place: the input planes are as they were
    if (!(filter.timings().average().seconds() > 0.0)) return 1;
    if (!write_file(argv[9], first)) return 2;
    const cv::Rect r = filter.filter_region();
    std::printf("apply 420 ok: region %d %d %d %d\n", r.x, r.y, r.width, r.height);
    return 0;
}
