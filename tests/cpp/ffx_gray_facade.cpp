// lvk::CASFilter and lvk::FSRFilter on one-channel (8UC1, GRAY) frames through the C++ facade: filter() dispatches on the frame's type, so both filters
// -- alone and behind a DeblockingFilter in a CompositeFilter -- take what the GRAY stabilizer push emits.
// usage: ffx_gray_facade <rows> <cols> <levels> <block> <k> <scaling> <multiplier> <sharpness> <in.bin> <out.bin>
//   in.bin: one tight frame; out.bin: CASFilter's output (the frame's size), FSRFilter's output (the frame's size times the multiplier), then that of
//   CompositeFilter{DeblockingFilter, FSRFilter, CASFilter} (the same size), all tight
#include <lvk/LiveVisionKit.hpp>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <vector>

#include "facade_util.hpp"

int main(int argc, char** argv)
{
    if (argc < 11) { std::fprintf(stderr, "usage\n"); return 2; }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]);
    lvk::DeblockingFilterSettings ds;
    ds.detection_levels = (uint32_t)std::atoi(argv[3]); ds.block_size = (uint32_t)std::atoi(argv[4]);
    ds.filter_size = (uint32_t)std::atoi(argv[5]); ds.filter_scaling = (float)std::atof(argv[6]);
    lvk::FSRFilterSettings fs;
    fs.size_multiplier = (float)std::atof(argv[7]);
    lvk::CASFilterSettings cs;
    cs.sharpness = (float)std::atof(argv[8]);
    std::vector<uint8_t> in((size_t)rows * cols), out;
    if (!read_file(argv[9], in)) return 2;
    FILE* f = std::fopen(argv[10], "wb");
    if (!f) return 2;
    auto emit = [&](const lvk::Frame& frame, uint64_t ts, const char* what) {
        if (frame.empty() || frame.type() != CV_8UC1 || frame.channels() != 1 || frame.format != lvk::VideoFrame::GRAY || frame.timestamp != ts)
        {
            std::fprintf(stderr, "%s: type, format or timestamp not carried through\n", what);
            return false;
        }
        out.resize((size_t)frame.cols * frame.rows);
        frame.download(out.data());
        std::printf("%s %dx%d\n", what, frame.cols, frame.rows);
        return std::fwrite(out.data(), 1, out.size(), f) == out.size();
    };

    lvk::CASFilter cas(cs);
    lvk::Frame frame;
    frame.upload(in.data(), rows, cols, lvk::VideoFrame::GRAY, 77);
    cas.apply(std::move(frame), frame);
    if (!emit(frame, 77, "CASFilter") || frame.cols != cols || frame.rows != rows) return 1;

    lvk::FSRFilter fsr(fs);
    lvk::Frame scaled;
    scaled.upload(in.data(), rows, cols, lvk::VideoFrame::GRAY, 78);
    fsr.apply(std::move(scaled), scaled);
    if (!emit(scaled, 78, "FSRFilter")) return 1;
    const int ow = scaled.cols, oh = scaled.rows;

    lvk::CompositeFilter chain({std::make_shared<lvk::DeblockingFilter>(ds), std::make_shared<lvk::FSRFilter>(fs), std::make_shared<lvk::CASFilter>(cs)});
    lvk::Frame again;
    again.upload(in.data(), rows, cols, lvk::VideoFrame::GRAY, 79);
    chain.apply(std::move(again), again);
    if (!emit(again, 79, "CompositeFilter") || again.cols != ow || again.rows != oh) return 1;
    std::fclose(f);

    // refused like the reference's asserts: a one-channel frame that does not say it is GRAY
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0;
    for (int k = 0; k < 2; k++)
    {
        lvk::Frame unknown;
        unknown.upload(in.data(), rows, cols, lvk::VideoFrame::GRAY, 80);
        unknown.format = lvk::VideoFrame::UNKNOWN;
        try
        {
            if (k == 0) cas.apply(std::move(unknown), unknown);
            else fsr.apply(std::move(unknown), unknown);
        }
        catch (const std::runtime_error&) { refused++; }
    }
    if (refused != 2) { std::fprintf(stderr, "%d of 2 refused\n", refused); return 1; }
    std::printf("ffx gray ok\n");
    return 0;
}
