// lvk::VideoFrameOBS and lvk::LCFilter::apply(VideoFrameOBS, VideoFrameOBS) of the C++ facade: the plugin's lens correction on the planes of any OBS
// video format in one call (lvk_hip_lens_apply_obs).
//
// lens_obs_facade <video format number> <test mode> <profile: "none" or nine numbers separated by commas> <rows> <cols> <in.bin> <out.bin>
//   in.bin / out.bin: the planes of the format one after the other, tightly packed.
#include <lvk/LiveVisionKit.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "facade_util.hpp"

int main(int argc, char** argv)
{
    if (argc != 8) { std::fprintf(stderr, "usage: see the head of lens_obs_facade.cpp\n"); return 2; }
    const int format = std::atoi(argv[1]);
    lvk::LCFilterSettings settings;
    settings.test_mode = std::atoi(argv[2]) != 0;
    if (std::strcmp(argv[3], "none") != 0)
    {
        double v[9]; char* p = argv[3];
        for (int i = 0; i < 9; i++) { v[i] = std::strtod(p, &p); if (*p == ',') p++; }
        lvk::CameraParameters c; c.fx = v[0]; c.fy = v[1]; c.cx = v[2]; c.cy = v[3]; c.k1 = v[4]; c.k2 = v[5]; c.p1 = v[6]; c.p2 = v[7]; c.k3 = v[8];
        settings.profile = c;
    }
    const int rows = std::atoi(argv[4]), cols = std::atoi(argv[5]);

    lvk::VideoFrameOBS input, output;
    input.create({cols, rows}, format);
    int prow[3], pbytes[3];
    const int n = lvk::VideoFrameOBS::plane_table(format, rows, cols, prow, pbytes);
    size_t total = 0;
    for (int i = 0; i < n; i++)
    {
        if (input.linesize[i] != pbytes[i] || input.data[i] != input.data[0] + total) return 1;
        total += (size_t)prow[i] * pbytes[i];
    }
    if (n == 0 || input.bytes() != total) return 1;
    std::vector<uint8_t> host(total), out(total), back(total), again(total);
    if (!read_file(argv[6], host)) return 2;
    input.upload(host.data(), rows, cols, format, 41);

    lvk::LCFilter filter(settings);
    filter.apply(input, output, true);
    if (output.empty() || output.rows != rows || output.cols != cols || output.format != format || output.timestamp != 41) return 1;
    if (output.data[0] == input.data[0] || output.context() != input.context() || output.bytes() != total) return 1;
    output.download(out.data());
    input.download(back.data());
    if (back != host) return 1;                                // out of place: the input planes are as they were, in test mode too
    if (!write_file(argv[7], out)) return 2;
    if (!(filter.timings().average().seconds() > 0.0)) return 1;

    // the same frame again, into the same output frame: the same bytes
    filter.apply(input, output);
    output.download(again.data());
    if (again != out) return 1;

    // refused like the reference's asserts: the input as its own output; a Y800 frame in test mode
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0;
    try { filter.apply(input, input); } catch (const std::runtime_error&) { refused++; }
    {
        lvk::LCFilterSettings grid; grid.test_mode = true;
        lvk::LCFilter f(grid);
        lvk::VideoFrameOBS gray, result;
        std::vector<uint8_t> g((size_t)rows * cols, 7);
        gray.upload(g.data(), rows, cols, LVK_VIDEO_FORMAT_Y800, 1);
        if (gray.bytes() != g.size()) return 1;
        try { f.apply(gray, result); } catch (const std::runtime_error&) { refused += result.empty() ? 1 : 0; }
    }
    if (refused != 2) { std::fprintf(stderr, "%d of 2 refused\n", refused); return 1; }
    std::printf("lens obs ok: %d %dx%d\n", format, cols, rows);
    return 0;
}
