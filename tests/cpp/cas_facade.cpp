// lvk::CASFilter of the C++ facade (include/lvk/CASFilter.hpp) driven the way a host of the plugin's filters would drive it.
//
// cas_facade apply <format> <rows> <cols> <sharpness> <frame.bin> <out.bin>
//   filter.apply(std::move(frame), frame): out of place into a fresh frame; checks that timestamp and format are kept.
// cas_facade chain <format> <rows> <cols> <sharpness> <frame.bin> <out.bin>
//   CompositeFilter{DeblockingFilter, CASFilter} with default deblocking settings: deblock, then sharpen.
// cas_facade --stream <obs format> <rows> <cols> <n frames> <sharpness> <planes.bin> <out.bin>
//   upload_obs_frame -> CASFilter::apply(std::move(frame), frame) -> download_ocl_frame; out.bin = the frames' tight planes.
// cas_facade configure
//   configure({1.5}) and CASFilter({-0.25}) must be refused (the assert handler throws); needs no device.
#include <lvk/LiveVisionKit.hpp>
#include <lvk/FrameIngest.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

struct fake_obs_source_frame            // the members of libobs' obs_source_frame the plugin's FrameIngest touches
{
    uint8_t* data[8] = {};
    uint32_t linesize[8] = {};
    uint32_t width = 0, height = 0;
    uint64_t timestamp = 0;
    int format = 0;
};

static bool read_file(const char* path, std::vector<uint8_t>& buf)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = std::fread(buf.data(), 1, buf.size(), f) == buf.size();
    std::fclose(f);
    return ok;
}

static bool write_file(const char* path, const std::vector<uint8_t>& buf)
{
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    std::fclose(f);
    return ok;
}

static int run_apply(char** argv, bool chain)
{
    const int fmt = std::atoi(argv[2]), rows = std::atoi(argv[3]), cols = std::atoi(argv[4]);
    lvk::CASFilterSettings s;
    s.sharpness = (float)std::atof(argv[5]);
    std::vector<uint8_t> host((size_t)rows * cols * 3);
    if (!read_file(argv[6], host)) return 2;

    auto cas = std::make_shared<lvk::CASFilter>(s);
    std::shared_ptr<lvk::VideoFilter> filter = cas;
    if (chain)
        filter = std::make_shared<lvk::CompositeFilter>(
            std::initializer_list<std::shared_ptr<lvk::VideoFilter>>{std::make_shared<lvk::DeblockingFilter>(), cas});
    lvk::Frame frame;
    frame.upload(host.data(), rows, cols, (lvk::VideoFrame::Format)fmt, 9);
    const void* before = frame.device_ptr();
    filter->apply(std::move(frame), frame);
    if (frame.empty() || frame.timestamp != 9 || frame.format != (lvk::VideoFrame::Format)fmt || frame.rows != rows || frame.cols != cols) return 1;
    if (!chain && frame.device_ptr() == before) return 1;          // a fresh frame, not the input's buffer
    frame.download(host.data());
    if (!write_file(argv[7], host)) return 2;
    std::printf("%s ok: %s\n", chain ? "chain" : "apply", filter->alias().c_str());
    return 0;
}

static int run_stream(char** argv)
{
    const int fmt = std::atoi(argv[2]), rows = std::atoi(argv[3]), cols = std::atoi(argv[4]), n = std::atoi(argv[5]);
    if (fmt != 1) return 2;                                  // I420
    lvk::CASFilterSettings s;
    s.sharpness = (float)std::atof(argv[6]);
    const size_t ybytes = (size_t)rows * cols, cbytes = (size_t)(rows / 2) * (cols / 2), frame_bytes = ybytes + 2 * cbytes;
    std::vector<uint8_t> clip(frame_bytes * n), back(frame_bytes), all;
    if (!read_file(argv[7], clip)) return 2;
    auto ingest = lvk::FrameIngest::Select(fmt);
    if (!ingest) return 1;
    lvk::CASFilter filter(s);
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
        if (frame.empty()) return 1;
        fake_obs_source_frame dst;
        dst.width = cols; dst.height = rows; dst.format = fmt;
        std::fill(back.begin(), back.end(), 0x5A);
        dst.data[0] = back.data(); dst.linesize[0] = cols;
        dst.data[1] = back.data() + ybytes; dst.linesize[1] = cols / 2;
        dst.data[2] = back.data() + ybytes + cbytes; dst.linesize[2] = cols / 2;
        ingest->download_ocl_frame(frame, &dst);
        all.insert(all.end(), back.begin(), back.end());
    }
    if (!write_file(argv[8], all)) return 2;
    std::printf("stream ok: %d frames\n", n);
    return 0;
}

static int run_configure()
{
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0;
    lvk::CASFilter filter;
    if (filter.settings().sharpness != 0.8f) return 1;
    try { filter.configure({1.5f}); } catch (const std::runtime_error&) { refused++; }
    try { lvk::CASFilter bad({-0.25f}); } catch (const std::runtime_error&) { refused++; }
    if (filter.settings().sharpness != 0.8f) return 1;             // a refused configure changes nothing
    filter.configure({1.0f});
    if (filter.settings().sharpness != 1.0f) return 1;
    std::printf("configure ok: %d refused, alias %s\n", refused, filter.alias().c_str());
    return refused == 2 ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc == 8 && std::string(argv[1]) == "apply") return run_apply(argv, false);
    if (argc == 8 && std::string(argv[1]) == "chain") return run_apply(argv, true);
    if (argc == 9 && std::string(argv[1]) == "--stream") return run_stream(argv);
    if (argc == 2 && std::string(argv[1]) == "configure") return run_configure();
    std::fprintf(stderr, "usage: see the head of cas_facade.cpp\n");
    return 2;
}
