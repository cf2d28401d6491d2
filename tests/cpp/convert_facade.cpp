// VideoFrame::reformat / reformatTo / viewAsFormat and lvk::ConversionFilter of the C++ facade (include/lvk/LiveVisionKit.hpp,
// include/lvk/ConversionFilter.hpp) driven the way a host of the plugin's filters would drive them.
//
// convert_facade frames <rows> <cols>
//   1-, 3- and 4-channel frames: create / type / channels / upload / download / clone, checked here byte for byte.
// convert_facade reformat <rows> <cols> <dir>
//   dir/in_<f>.bin holds a frame of format f (0..5); for every (src, dst) pair reformatTo writes dir/to_<src>_<dst>.bin, reformat (in place)
//   writes dir/re_<src>_<dst>.bin, viewAsFormat writes dir/view_<src>_<dst>.bin.  Timestamps, formats and the buffer sharing of the
//   same-format cases are checked here.
// convert_facade filter <rows> <cols> <dir>
//   every supported (code, source format, output channels) through ConversionFilter::apply(std::move(frame), frame); writes
//   dir/cf_<code>_<src>_<dcn>.bin and prints "cf <code> <src> <dcn> <format>" per case.
// convert_facade chain <rows> <cols> <sharpness> <yuv.bin> <out.bin>
//   CompositeFilter{ConversionFilter(YUV2BGR), CASFilter, ConversionFilter(BGR2YUV)} on a YUV frame.
// convert_facade --stream <rows> <cols> <n frames> <planes.bin> <out.bin>
//   the plugin's export step: I420 through FrameIngest::upload_obs_frame, then viewAsFormat(RGBA); out.bin = the RGBA frames.
// convert_facade configure
//   unsupported codes / output channels must be refused (the assert handler throws); needs no device.
#include <lvk/LiveVisionKit.hpp>
#include <lvk/FrameIngest.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "facade_util.hpp"

using Format = lvk::VideoFrame::Format;

static std::vector<uint8_t> download(const lvk::VideoFrame& f)
{
    std::vector<uint8_t> host((size_t)f.rows * f.cols * f.channels());
    f.download(host.data());
    return host;
}

static int run_frames(char** argv)
{
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    const Format fmts[3] = {lvk::VideoFrame::GRAY, lvk::VideoFrame::YUV, lvk::VideoFrame::RGBA};
    const int types[3] = {CV_8UC1, CV_8UC3, CV_8UC4};
    for (int k = 0; k < 3; k++)
    {
        const int ch = k == 0 ? 1 : k == 1 ? 3 : 4;
        std::vector<uint8_t> host((size_t)rows * cols * ch);
        for (size_t i = 0; i < host.size(); i++) host[i] = (uint8_t)(i * 131 + 7 * k + (i >> 9));
        lvk::VideoFrame made;
        made.create({cols, rows}, types[k]);
        if (made.type() != types[k] || made.channels() != ch || made.step != (size_t)cols * ch) return 10 + k;
        lvk::Frame frame;
        frame.upload(host.data(), rows, cols, fmts[k], 40 + k);
        if (frame.type() != types[k] || frame.channels() != ch || frame.step != (size_t)cols * ch || frame.format != fmts[k]) return 20 + k;
        lvk::VideoFrame copy = frame.clone();
        if (copy.device_ptr() == frame.device_ptr() || copy.type() != types[k] || copy.timestamp != 40u + k || copy.format != fmts[k]) return 30 + k;
        if (download(frame) != host || download(copy) != host) return 40 + k;
        // re-creating at another channel count reallocates; at the same one it keeps the buffer
        const void* before = frame.device_ptr();
        frame.create({cols, rows}, types[k]);
        if (frame.device_ptr() != before) return 50 + k;
        frame.create({cols, rows}, types[(k + 1) % 3]);
        if (frame.channels() == ch || frame.step != (size_t)cols * frame.channels()) return 60 + k;
    }
    std::printf("frames ok\n");
    return 0;
}

static int run_reformat(char** argv)
{
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    const std::string dir = argv[4];
    for (int s = 0; s < 6; s++)
    {
        std::vector<uint8_t> host((size_t)rows * cols * lvk::VideoFrame::channels_of((Format)s));
        if (!read_file(dir + "/in_" + std::to_string(s) + ".bin", host)) return 2;
        lvk::Frame src;
        src.upload(host.data(), rows, cols, (Format)s, 100 + s);
        for (int d = 0; d < 6; d++)
        {
            const std::string tag = std::to_string(s) + "_" + std::to_string(d);
            lvk::VideoFrame to(7);
            src.reformatTo(to, (Format)d);
            if (to.format != (Format)d || to.timestamp != 100u + s || to.channels() != lvk::VideoFrame::channels_of((Format)d)) return 10;
            if (to.device_ptr() == src.device_ptr()) return 11;                    // a copy when the format stays
            if (!write_file(dir + "/to_" + tag + ".bin", download(to))) return 2;

            lvk::Frame re = src.clone();
            const void* before = re.device_ptr();
            re.reformat((Format)d);
            if (re.format != (Format)d || re.timestamp != 100u + s) return 12;
            if ((s == d) != (re.device_ptr() == before)) return 13;               // the same format does nothing
            if (!write_file(dir + "/re_" + tag + ".bin", download(re))) return 2;

            lvk::VideoFrame view;
            src.viewAsFormat(view, (Format)d);
            if (view.format != (Format)d || view.timestamp != 100u + s) return 14;
            if ((s == d) != (view.device_ptr() == src.device_ptr())) return 15;     // the same format shares the buffer
            if (!write_file(dir + "/view_" + tag + ".bin", download(view))) return 2;
        }
        if (download(src) != host) return 16;                                     // the source is only read
    }
    std::printf("reformat ok: 36 pairs\n");
    return 0;
}

static int run_filter(char** argv)
{
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    const std::string dir = argv[4];
    const int codes[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 82, 83, 84, 85};
    int cases = 0;
    for (int code : codes)
        for (int s = 0; s < 6; s++)
            for (int dcn = 0; dcn <= 4; dcn++)
            {
                const int to = lvk_hip_cvt_code_target(code, s, dcn);
                if (to < 0 || (dcn != 0 && dcn != 4)) continue;                     // output_channels: none, and 4 where a code takes it
                std::vector<uint8_t> host((size_t)rows * cols * lvk::VideoFrame::channels_of((Format)s));
                if (!read_file(dir + "/in_" + std::to_string(s) + ".bin", host)) return 2;
                lvk::ConversionFilterSettings settings;
                settings.conversion_code = (cv::ColorConversionCodes)code;
                if (dcn) settings.output_channels = (size_t)dcn;
                lvk::ConversionFilter filter(settings);
                lvk::Frame frame;
                frame.upload(host.data(), rows, cols, (Format)s, 900 + code);
                filter.apply(std::move(frame), frame);
                if (frame.empty() || frame.timestamp != 900u + code || frame.format != (Format)to) return 10;
                if (frame.channels() != lvk::VideoFrame::channels_of((Format)to)) return 11;
                if (!write_file(dir + "/cf_" + std::to_string(code) + "_" + std::to_string(s) + "_" + std::to_string(dcn) + ".bin", download(frame)))
                    return 2;
                std::printf("cf %d %d %d %d\n", code, s, dcn, to);
                cases++;
            }
    std::printf("filter ok: %d cases, %s\n", cases, lvk::ConversionFilter().alias().c_str());
    return 0;
}

static int run_chain(char** argv)
{
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    lvk::CASFilterSettings s;
    s.sharpness = (float)std::atof(argv[4]);
    std::vector<uint8_t> host((size_t)rows * cols * 3);
    if (!read_file(argv[5], host)) return 2;
    lvk::CompositeFilter chain(std::initializer_list<std::shared_ptr<lvk::VideoFilter>>{
        std::make_shared<lvk::ConversionFilter>(cv::COLOR_YUV2BGR), std::make_shared<lvk::CASFilter>(s),
        std::make_shared<lvk::ConversionFilter>(cv::COLOR_BGR2YUV)});
    lvk::Frame frame;
    frame.upload(host.data(), rows, cols, lvk::VideoFrame::YUV, 31);
    chain.apply(std::move(frame), frame);
    if (frame.empty() || frame.timestamp != 31 || frame.format != lvk::VideoFrame::YUV || frame.channels() != 3) return 1;
    if (!write_file(argv[6], download(frame))) return 2;
    std::printf("chain ok: %s\n", chain.alias().c_str());
    return 0;
}

static int run_stream(char** argv)
{
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), n = std::atoi(argv[4]);
    const size_t ybytes = (size_t)rows * cols, cbytes = (size_t)(rows / 2) * (cols / 2), frame_bytes = ybytes + 2 * cbytes;
    std::vector<uint8_t> clip(frame_bytes * n), all;
    if (!read_file(argv[5], clip)) return 2;
    auto ingest = lvk::FrameIngest::Select(1);               // I420
    if (!ingest) return 1;
    lvk::Frame frame;
    lvk::VideoFrame rgba;
    for (int k = 0; k < n; k++)
    {
        fake_obs_source_frame obs;
        obs.width = cols; obs.height = rows; obs.format = 1; obs.timestamp = 500 + k;
        uint8_t* p = clip.data() + frame_bytes * k;
        obs.data[0] = p; obs.linesize[0] = cols;
        obs.data[1] = p + ybytes; obs.linesize[1] = cols / 2;
        obs.data[2] = p + ybytes + cbytes; obs.linesize[2] = cols / 2;
        ingest->upload_obs_frame(&obs, frame);
        frame.viewAsFormat(rgba, lvk::VideoFrame::RGBA);      // OBSFrame::to_obs_texture's RGBA view
        if (rgba.format != lvk::VideoFrame::RGBA || rgba.channels() != 4 || rgba.timestamp != frame.timestamp) return 1;
        const std::vector<uint8_t> host = download(rgba);
        all.insert(all.end(), host.begin(), host.end());
    }
    if (!write_file(argv[6], all)) return 2;
    std::printf("stream ok: %d frames\n", n);
    return 0;
}

static int run_configure()
{
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0;
    lvk::ConversionFilter filter;
    if (filter.settings().conversion_code != cv::COLOR_BGR2YUV || filter.settings().output_channels) return 1;
    try { filter.configure({(cv::ColorConversionCodes)40, std::nullopt}); } catch (const std::runtime_error&) { refused++; }       // BGR2HSV
    try { filter.configure({(cv::ColorConversionCodes)127, std::nullopt}); } catch (const std::runtime_error&) { refused++; }      // YUV2RGB_I420
    try { filter.configure({cv::COLOR_BGR2YUV, 4}); } catch (const std::runtime_error&) { refused++; }
    try { filter.configure({cv::COLOR_BGR2GRAY, 3}); } catch (const std::runtime_error&) { refused++; }
    try { filter.configure({cv::COLOR_YUV2BGR, (size_t)1 << 33}); } catch (const std::runtime_error&) { refused++; }
    try { lvk::ConversionFilter bad((cv::ColorConversionCodes)-1); } catch (const std::runtime_error&) { refused++; }
    if (filter.settings().conversion_code != cv::COLOR_BGR2YUV || filter.settings().output_channels) return 1;   // refused: nothing changes
    filter.configure({cv::COLOR_YUV2RGB, 4});
    if (filter.settings().conversion_code != cv::COLOR_YUV2RGB || filter.settings().output_channels != 4u) return 1;
    // the 3-channel VideoFrame metadata needs no device
    lvk::VideoFrame empty;
    if (empty.type() != CV_8UC3 || empty.channels() != 3 || lvk::VideoFrame::channels_of(lvk::VideoFrame::BGRA) != 4) return 1;
    std::printf("configure ok: %d refused, alias %s\n", refused, filter.alias().c_str());
    return refused == 6 ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc == 4 && std::string(argv[1]) == "frames") return run_frames(argv);
    if (argc == 5 && std::string(argv[1]) == "reformat") return run_reformat(argv);
    if (argc == 5 && std::string(argv[1]) == "filter") return run_filter(argv);
    if (argc == 7 && std::string(argv[1]) == "chain") return run_chain(argv);
    if (argc == 7 && std::string(argv[1]) == "--stream") return run_stream(argv);
    if (argc == 2 && std::string(argv[1]) == "configure") return run_configure();
    std::fprintf(stderr, "usage: see the head of convert_facade.cpp\n");
    return 2;
}
