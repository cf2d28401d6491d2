// lvk::FSRFilter of the C++ facade (include/lvk/FSRFilter.hpp) driven the way a host of the plugin's filters would drive it.
//
// fsr_facade apply <format> <rows> <cols> <out rows> <out cols> <multiplier> <aspect> <l> <t> <r> <b> <frame.bin> <out.bin>
//   filter.apply(std::move(frame), frame); prints the output size; checks that timestamp and format are kept.
// fsr_facade chain <same arguments>
//   CompositeFilter{FSRFilter, CASFilter} with CAS at its default sharpness (0.8): scale, then sharpen.
// fsr_facade --stream <obs format> <rows> <cols> <n frames> <multiplier> <planes.bin> <out.bin>
//   upload_obs_frame -> FSRFilter::apply(std::move(frame), frame) -> download_ocl_frame into an output-sized frame; out.bin = its planes.
// fsr_facade configure
//   bad crops, multipliers and sizes must be refused (the assert handler throws); needs no device.
#include <lvk/LiveVisionKit.hpp>
#include <lvk/FrameIngest.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "facade_util.hpp"

static int channels_of(int fmt) { return fmt == 1 || fmt == 3 ? 4 : 3; }

static int run_apply(char** argv, bool chain)
{
    const int fmt = std::atoi(argv[2]), rows = std::atoi(argv[3]), cols = std::atoi(argv[4]);
    lvk::FSRFilterSettings s;
    s.output_size = cv::Size(std::atoi(argv[6]), std::atoi(argv[5]));
    s.size_multiplier = (float)std::atof(argv[7]);
    s.maintain_aspect_ratio = std::atoi(argv[8]) != 0;
    s.crop_left = std::atoi(argv[9]); s.crop_top = std::atoi(argv[10]); s.crop_right = std::atoi(argv[11]); s.crop_bottom = std::atoi(argv[12]);
    const int ch = channels_of(fmt);
    std::vector<uint8_t> host((size_t)rows * cols * ch);
    if (!read_file(argv[13], host)) return 2;

    auto fsr = std::make_shared<lvk::FSRFilter>(s);
    std::shared_ptr<lvk::VideoFilter> filter = fsr;
    if (chain)
        filter = std::make_shared<lvk::CompositeFilter>(
            std::initializer_list<std::shared_ptr<lvk::VideoFilter>>{fsr, std::make_shared<lvk::CASFilter>()});
    lvk::Frame frame;
    frame.upload(host.data(), rows, cols, (lvk::VideoFrame::Format)fmt, 9);
    filter->apply(std::move(frame), frame);
    if (frame.empty() || frame.timestamp != 9 || frame.format != (lvk::VideoFrame::Format)fmt) return 1;
    std::vector<uint8_t> out((size_t)frame.rows * frame.cols * ch);
    frame.download(out.data());
    if (!write_file(argv[14], out)) return 2;
    std::printf("%s ok: %s %dx%d\n", chain ? "chain" : "apply", filter->alias().c_str(), frame.rows, frame.cols);
    return 0;
}

static int run_stream(char** argv)
{
    const int fmt = std::atoi(argv[2]), rows = std::atoi(argv[3]), cols = std::atoi(argv[4]), n = std::atoi(argv[5]);
    if (fmt != 1) return 2;                                  // I420
    lvk::FSRFilterSettings s;
    s.size_multiplier = (float)std::atof(argv[6]);
    const int orows = (int)std::nearbyint(rows * s.size_multiplier), ocols = (int)std::nearbyint(cols * s.size_multiplier);
    const size_t ybytes = (size_t)rows * cols, cbytes = (size_t)(rows / 2) * (cols / 2), frame_bytes = ybytes + 2 * cbytes;
    const size_t oybytes = (size_t)orows * ocols, ocbytes = (size_t)(orows / 2) * (ocols / 2), oframe_bytes = oybytes + 2 * ocbytes;
    std::vector<uint8_t> clip(frame_bytes * n), back(oframe_bytes), all;
    if (!read_file(argv[7], clip)) return 2;
    auto ingest = lvk::FrameIngest::Select(fmt);
    if (!ingest) return 1;
    lvk::FSRFilter filter(s);
    lvk::Frame frame;
    for (int k = 0; k < n; k++)
    {
        fake_obs_source_frame obs;
        obs.width = cols; obs.height = rows; obs.format = fmt; obs.timestamp = 500 + k;
        uint8_t* p = clip.data() + frame_bytes * k;
        obs.data[0] = p; obs.linesize[0] = cols;
        obs.data[1] = p + ybytes; obs.linesize[1] = cols / 2;
        obs.data[2] = p + ybytes + cbytes; obs.linesize[2] = cols / 2;
        ingest->upload_obs_frame(&obs, frame);
        filter.apply(std::move(frame), frame);
        if (frame.empty() || frame.rows != orows || frame.cols != ocols) return 1;
        fake_obs_source_frame dst;
        dst.width = ocols; dst.height = orows; dst.format = fmt;
        std::fill(back.begin(), back.end(), 0x5A);
        dst.data[0] = back.data(); dst.linesize[0] = ocols;
        dst.data[1] = back.data() + oybytes; dst.linesize[1] = ocols / 2;
        dst.data[2] = back.data() + oybytes + ocbytes; dst.linesize[2] = ocols / 2;
        ingest->download_ocl_frame(frame, &dst);
        all.insert(all.end(), back.begin(), back.end());
    }
    if (!write_file(argv[8], all)) return 2;
    std::printf("stream ok: %d frames %dx%d\n", n, orows, ocols);
    return 0;
}

static int run_configure()
{
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0;
    lvk::FSRFilter filter;
    if (filter.settings().size_multiplier != 1.0f || !filter.settings().maintain_aspect_ratio) return 1;
    lvk::FSRFilterSettings bad[6];
    bad[0].crop_left = -1;
    bad[1].crop_bottom = 4097;
    bad[2].size_multiplier = 0.0f;
    bad[3].size_multiplier = NAN;
    bad[4].output_size = cv::Size(-1, 10);
    bad[5].output_size = cv::Size(10, -1);
    for (const auto& b : bad)
        try { filter.configure(b); } catch (const std::runtime_error&) { refused++; }
    try { lvk::FSRFilter f(bad[0]); } catch (const std::runtime_error&) { refused++; }
    if (filter.settings().size_multiplier != 1.0f || filter.settings().crop_left != 0) return 1;     // a refused configure changes nothing
    lvk::FSRFilterSettings good;
    good.crop_top = 4096;
    good.output_size = cv::Size(3840, 2160);
    filter.configure(good);
    if (filter.settings().crop_top != 4096 || filter.settings().output_size.width != 3840) return 1;
    std::printf("configure ok: %d refused, alias %s\n", refused, filter.alias().c_str());
    return refused == 7 ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc == 15 && std::string(argv[1]) == "apply") return run_apply(argv, false);
    if (argc == 15 && std::string(argv[1]) == "chain") return run_apply(argv, true);
    if (argc == 9 && std::string(argv[1]) == "--stream") return run_stream(argv);
    if (argc == 2 && std::string(argv[1]) == "configure") return run_configure();
    std::fprintf(stderr, "usage: see the head of fsr_facade.cpp\n");
    return 2;
}
