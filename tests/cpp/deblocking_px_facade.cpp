// lvk::DeblockingFilter on one-channel (8UC1, GRAY) and four-channel (8UC4, BGRA) frames through the C++ facade: filter() dispatches on the frame's type,
// so the filter -- alone and ahead of a ScalingFilter in a CompositeFilter -- takes what the GRAY and four-channel stabilizer pushes emit.
// usage: deblocking_px_facade <rows> <cols> <channels: 1 | 4> <levels> <block> <k> <scaling> <out width> <out height> <in.bin> <out.bin>
//   in.bin: one tight frame; out.bin: DeblockingFilter's output (the frame's size), then that of CompositeFilter{DeblockingFilter, ScalingFilter(size, 0.8)}
//   (the output size), both tight
#include <lvk/LiveVisionKit.hpp>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <vector>

#include "facade_util.hpp"

int main(int argc, char** argv)
{
    if (argc < 12) { std::fprintf(stderr, "usage\n"); return 2; }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), ch = std::atoi(argv[3]), ow = std::atoi(argv[8]), oh = std::atoi(argv[9]);
    if (ch != 1 && ch != 4) return 2;
    lvk::DeblockingFilterSettings s;
    s.detection_levels = (uint32_t)std::atoi(argv[4]); s.block_size = (uint32_t)std::atoi(argv[5]);
    s.filter_size = (uint32_t)std::atoi(argv[6]); s.filter_scaling = (float)std::atof(argv[7]);
    const lvk::VideoFrame::Format fmt = ch == 1 ? lvk::VideoFrame::GRAY : lvk::VideoFrame::BGRA;
    const int type = ch == 1 ? CV_8UC1 : CV_8UC4;
    std::vector<uint8_t> in((size_t)rows * cols * ch), out;
    if (!read_file(argv[10], in)) return 2;
    FILE* f = std::fopen(argv[11], "wb");
    if (!f) return 2;
    auto emit = [&](const lvk::Frame& frame, uint64_t ts, int w, int h, const char* what) {
        if (frame.empty() || frame.type() != type || frame.channels() != ch || frame.format != fmt || frame.timestamp != ts || frame.cols != w || frame.rows != h)
        {
            std::fprintf(stderr, "%s: type, format, timestamp or size not carried through\n", what);
            return false;
        }
        out.resize((size_t)w * h * ch);
        frame.download(out.data());
        return std::fwrite(out.data(), 1, out.size(), f) == out.size();
    };

    lvk::DeblockingFilter deblocker(s);
    lvk::Frame frame;
    frame.upload(in.data(), rows, cols, fmt, 77);
    deblocker.apply(std::move(frame), frame);
    if (!emit(frame, 77, cols, rows, "DeblockingFilter")) return 1;
    const cv::Rect r = deblocker.filter_region();

    auto first = std::make_shared<lvk::DeblockingFilter>(s);
    auto second = std::make_shared<lvk::ScalingFilter>(cv::Size(ow, oh), 0.8f);
    lvk::CompositeFilter chain({first, second});
    lvk::Frame again;
    again.upload(in.data(), rows, cols, fmt, 78);
    chain.apply(std::move(again), again);
    if (!emit(again, 78, ow, oh, "CompositeFilter")) return 1;
    std::fclose(f);

    // refused like the reference's asserts: a four-channel frame of unknown format (which byte is blue?), and the influence overlay on anything but 8UC3
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0;
    lvk::Frame unknown;
    unknown.upload(std::vector<uint8_t>((size_t)rows * cols * 4).data(), rows, cols, lvk::VideoFrame::BGRA, 79);
    unknown.format = lvk::VideoFrame::UNKNOWN;
    try { deblocker.apply(std::move(unknown), unknown); } catch (const std::runtime_error&) { refused++; }
    lvk::Frame overlay;
    overlay.upload(in.data(), rows, cols, fmt, 80);
    try { deblocker.draw_influence(overlay); } catch (const std::runtime_error&) { refused++; }
    const cv::Rect after = deblocker.filter_region();
    if (refused != 2 || after.width != r.width || after.height != r.height) { std::fprintf(stderr, "%d of 2 refused\n", refused); return 1; }
    std::printf("deblocking ok: %d channel(s) %dx%d, region %d %d %d %d\n", ch, cols, rows, r.x, r.y, r.width, r.height);
    return 0;
}
