// lvk::ScalingFilter on one-channel (8UC1, GRAY) and four-channel (8UC4, BGRA) frames through the C++ facade: lvk::upscale and lvk::sharpen dispatch on the
// frame's type, so the filter -- alone and inside a CompositeFilter -- takes what the GRAY and four-channel stabilizer pushes emit.
// usage: scaling_px_facade <rows> <cols> <out width> <out height> <channels: 1 | 4> <sharpness> <in.bin> <out.bin>
//   in.bin: one tight frame; out.bin: ScalingFilter's output, then that of CompositeFilter{ScalingFilter(size, sharpness), ScalingFilter(size, 0.3)}
//   (whose second stage upscales to the size it is given: a copy, then RCAS), both tight
#include <lvk/LiveVisionKit.hpp>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "facade_util.hpp"

int main(int argc, char** argv)
{
    if (argc < 9) { std::fprintf(stderr, "usage\n"); return 2; }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), ow = std::atoi(argv[3]), oh = std::atoi(argv[4]), ch = std::atoi(argv[5]);
    const float sharpness = (float)std::atof(argv[6]);
    if (ch != 1 && ch != 4) return 2;
    const lvk::VideoFrame::Format fmt = ch == 1 ? lvk::VideoFrame::GRAY : lvk::VideoFrame::BGRA;
    const int type = ch == 1 ? CV_8UC1 : CV_8UC4;
    std::vector<uint8_t> in((size_t)rows * cols * ch), out((size_t)oh * ow * ch);
    if (!read_file(argv[7], in)) return 2;
    FILE* f = std::fopen(argv[8], "wb");
    if (!f) return 2;
    auto emit = [&](const lvk::Frame& frame, uint64_t ts, const char* what) {
        if (frame.empty() || frame.type() != type || frame.channels() != ch || frame.format != fmt || frame.timestamp != ts || frame.cols != ow || frame.rows != oh)
        {
            std::fprintf(stderr, "%s: type, format, timestamp or size not carried through\n", what);
            return false;
        }
        frame.download(out.data());
        return std::fwrite(out.data(), 1, out.size(), f) == out.size();
    };

    lvk::ScalingFilterSettings settings;                    // yuv_input stays at its default, true: it is not looked at for these frames
    settings.output_size = cv::Size(ow, oh); settings.sharpness = sharpness;
    lvk::ScalingFilter scaler(settings);
    lvk::Frame frame;
    frame.upload(in.data(), rows, cols, fmt, 77);
    scaler.apply(std::move(frame), frame);
    if (!emit(frame, 77, "ScalingFilter")) return 1;

    auto first = std::make_shared<lvk::ScalingFilter>(settings);
    auto second = std::make_shared<lvk::ScalingFilter>(cv::Size(ow, oh), 0.3f);
    lvk::CompositeFilter chain({first, second});
    lvk::Frame again;
    again.upload(in.data(), rows, cols, fmt, 78);
    chain.apply(std::move(again), again);
    if (!emit(again, 78, "CompositeFilter")) return 1;
    std::fclose(f);
    std::printf("scaling ok: %d channel(s) %dx%d -> %dx%d\n", ch, cols, rows, ow, oh);
    return 0;
}
