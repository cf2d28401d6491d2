// lvk::LCFilter of the C++ facade (include/lvk/LCFilter.hpp): the plugin's lens correction on packed frames and on I420 / NV12 planes.
//
// lc_filter_facade <mode> <test mode> <profile: "none" or nine numbers separated by commas> <rows> <cols> <in.bin> <out.bin> [<rows2> <cols2> <in2.bin> <out2.bin>]
//   mode: i420 | nv12 (tight planes through apply(VideoFrame420, VideoFrame420)), bgr | gray (a packed frame through apply(VideoFrame, VideoFrame)),
//   composite (the BGR frame through a CompositeFilter that holds the filter).  With the second size the same filter takes a frame of that size next and
//   the first one again, whose output must repeat: the map follows the frame size.
#include <lvk/LiveVisionKit.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "facade_util.hpp"

namespace {

bool planes_through(lvk::LCFilter& filter, bool nv12, int rows, int cols, const std::vector<uint8_t>& host, std::vector<uint8_t>& out, uint64_t ts)
{
    std::vector<uint8_t> back(host.size());
    lvk::VideoFrame420 input, output;
    input.upload(host.data(), rows, cols, nv12, ts);
    filter.apply(input, output, true);
    if (output.empty() || output.rows != rows || output.cols != cols || output.nv12 != nv12 || output.timestamp != ts) return false;
    if (output.y() == input.y() || output.context() != input.context()) return false;
    out.resize(host.size());
    output.download(out.data());
    input.download(back.data());
    return back == host;                                       // out of place: the input planes are as they were, in test mode too
}

bool frame_through(lvk::VideoFilter& filter, lvk::VideoFrame::Format format, int rows, int cols, const std::vector<uint8_t>& host, std::vector<uint8_t>& out, uint64_t ts)
{
    lvk::VideoFrame input, output;
    input.upload(host.data(), rows, cols, format, ts);
    filter.apply(std::move(input), output, true);
    if (output.empty() || output.rows != rows || output.cols != cols || output.format != format || output.timestamp != ts) return false;
    out.resize(host.size());
    output.download(out.data());
    return true;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 8 && argc != 12) { std::fprintf(stderr, "usage: see the head of lc_filter_facade.cpp\n"); return 2; }
    const std::string mode = argv[1];
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
    const bool planar = mode == "i420" || mode == "nv12", gray = mode == "gray";
    const size_t bytes = planar ? (size_t)rows * cols * 3 / 2 : (size_t)rows * cols * (gray ? 1 : 3);
    std::vector<uint8_t> host(bytes), first, again;
    if (!read_file(argv[6], host)) return 2;

    auto filter = std::make_shared<lvk::LCFilter>(settings);
    lvk::CompositeFilter composite({filter});
    const lvk::VideoFrame::Format format = gray ? lvk::VideoFrame::GRAY : lvk::VideoFrame::BGR;
    const auto once = [&](int r, int c, const std::vector<uint8_t>& in, std::vector<uint8_t>& out, uint64_t ts) {
        if (planar) return planes_through(*filter, mode == "nv12", r, c, in, out, ts);
        if (mode == "composite") return frame_through(composite, format, r, c, in, out, ts);
        return frame_through(*filter, format, r, c, in, out, ts);
    };
    if (!once(rows, cols, host, first, 41)) return 1;
    if (!write_file(argv[7], first)) return 2;
    if (!(filter->timings().average().seconds() > 0.0)) return 1;

    // the view region: the whole frame without a profile, inside the frame with one
    const cv::Rect view = filter->view_region(cv::Size(cols, rows));
    if (!settings.profile && (view.x != 0 || view.y != 0 || view.width != cols || view.height != rows)) return 1;
    if (view.width <= 0 || view.height <= 0 || view.x + view.width > cols || view.y + view.height > rows) return 1;

    if (argc == 12)
    {
        const int rows2 = std::atoi(argv[8]), cols2 = std::atoi(argv[9]);
        std::vector<uint8_t> host2(planar ? (size_t)rows2 * cols2 * 3 / 2 : (size_t)rows2 * cols2 * (gray ? 1 : 3)), second;
        if (!read_file(argv[10], host2)) return 2;
        if (!once(rows2, cols2, host2, second, 42)) return 1;
        if (!write_file(argv[11], second)) return 2;
        if (!once(rows, cols, host, again, 43) || again != first) return 1;
    }

    // refused like the reference's asserts: a profile with a zero focal length; the test mode on a one-channel frame; the input as its own output
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0;
    {
        lvk::LCFilterSettings bad = settings;
        bad.profile = lvk::CameraParameters{};
        try { filter->configure(bad); } catch (const std::runtime_error&) { refused++; }
        lvk::LCFilterSettings grid; grid.test_mode = true;
        lvk::LCFilter f(grid);
        lvk::VideoFrame in, out;
        std::vector<uint8_t> g((size_t)rows * cols, 7);
        in.upload(g.data(), rows, cols, lvk::VideoFrame::GRAY, 1);
        try { f.apply(std::move(in), out); } catch (const std::runtime_error&) { refused += out.empty() ? 1 : 0; }
        if (planar)
        {
            lvk::VideoFrame420 io;
            io.upload(host.data(), rows, cols, mode == "nv12", 1);
            try { filter->apply(io, io); } catch (const std::runtime_error&) { refused++; }
        }
        else refused++;
    }
    if (refused != 3) { std::fprintf(stderr, "%d of 3 refused\n", refused); return 1; }
    // the refused configure left the filter as it was
    if (!once(rows, cols, host, again, 44) || again != first) return 1;
    std::printf("lc filter ok: %s %dx%d view %d %d %d %d\n", mode.c_str(), cols, rows, view.x, view.y, view.width, view.height);
    return 0;
}
