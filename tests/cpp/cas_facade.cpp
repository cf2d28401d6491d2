// lvk::CASFilter of the C++ facade (include/lvk/CASFilter.hpp) driven the way a host of the plugin's filters would drive it.
//
// cas_facade apply <format> <rows> <cols> <sharpness> <frame.bin> <out.bin>
//   filter.apply(std::move(frame), frame): out of place into a fresh frame; checks that timestamp and format are kept.
// cas_facade chain <format> <rows> <cols> <sharpness> <frame.bin> <out.bin>
//   CompositeFilter{DeblockingFilter, CASFilter} with default deblocking settings: deblock, then sharpen.
// cas_facade --stream <obs format> <rows> <cols> <n frames> <sharpness> <planes.bin> <out.bin>
//   upload_obs_frame -> CASFilter::apply(std::move(frame), frame) -> download_ocl_frame; out.bin = the frames' tight planes.
// cas_facade cross <sharpness>
//   two CASFilters on contexts A and B, each fed frames of the other's context from its own thread; the outputs must equal single-threaded runs.
// cas_facade configure
//   configure({1.5}) and CASFilter({-0.25}) must be refused (the assert handler throws); needs no device.
#include <lvk/LiveVisionKit.hpp>
#include <lvk/FrameIngest.hpp>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "facade_util.hpp"

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

// The cross-context fences take both contexts' locks (Context::wait_for).  Taken while a filter still holds its own lock, two filters on
// contexts A and B, fed from two threads with frames of each other's context, each keep their own mutex while waiting for the other's.  A
// filter adopts the context of its first frame, so each is primed with a frame of its own.  A watchdog turns a hang into a failure.
static int run_cross(char** argv)
{
    const int rows = 36, cols = 64, n = 2000, distinct = 16;      // small frames, many applies: the window is microseconds wide
    const lvk::CASFilterSettings s{(float)std::atof(argv[2])};
    std::vector<uint8_t> pixels[2][distinct];
    for (int t = 0; t < 2; t++)
        for (int i = 0; i < distinct; i++)
        {
            pixels[t][i].resize((size_t)rows * cols * 3);
            for (size_t k = 0; k < pixels[t][i].size(); k++) pixels[t][i][k] = (uint8_t)((k * (5 + 2 * t) + 31 * i) % 251);
        }
    using Ctx = std::shared_ptr<lvk::hip::Context>;
    using Outputs = std::vector<std::vector<uint8_t>>;
    // thread t: a filter primed on filter_ctx, then fed frames uploaded on frames_ctx; one output in a hundred is kept (a download synchronises)
    auto feed = [&](int t, const Ctx& frames_ctx, const Ctx& filter_ctx, Outputs& outs) {
        lvk::CASFilter filter(s);
        lvk::Frame frame;
        frame.upload(pixels[t][0].data(), rows, cols, lvk::VideoFrame::BGR, 0, filter_ctx);
        filter.apply(std::move(frame), frame);
        for (int i = 0; i < n; i++)
        {
            frame.upload(pixels[t][i % distinct].data(), rows, cols, lvk::VideoFrame::BGR, i, frames_ctx);
            filter.apply(std::move(frame), frame);
            if (i % 100 != 99) continue;
            outs.emplace_back(pixels[t][0].size());
            frame.download(outs.back().data());
        }
    };
    Outputs want[2];
    for (int t = 0; t < 2; t++) { auto c = std::make_shared<lvk::hip::Context>(); feed(t, c, c, want[t]); }
    if (want[0].size() != (size_t)n / 100 || want[0][5] == want[1][5]) { std::printf("cross: reference runs implausible\n"); return 1; }
    for (int round = 0; round < 3; round++)
    {
        auto A = std::make_shared<lvk::hip::Context>(), B = std::make_shared<lvk::hip::Context>();
        Outputs got[2];
        std::atomic<int> done{0};
        std::thread t0([&] { feed(0, B, A, got[0]); done++; });          // filter on A, frames on B
        std::thread t1([&] { feed(1, A, B, got[1]); done++; });          // filter on B, frames on A
        for (int ms = 0; ms < 60000 && done.load() < 2; ms += 5) std::this_thread::sleep_for(std::chrono::milliseconds(5));
        if (done.load() < 2) { std::printf("cross: DEADLOCK (two CASFilters on two contexts feeding each other, round %d)\n", round); std::fflush(stdout); std::_Exit(1); }
        t0.join(); t1.join();
        for (int t = 0; t < 2; t++)
            if (got[t] != want[t]) { std::printf("cross: thread %d's outputs differ from its single-threaded run (round %d)\n", t, round); return 1; }
    }
    std::printf("cross ok: 2 CASFilters on 2 contexts feeding each other from 2 threads: no deadlock, bytes equal\n");
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
    if (argc == 3 && std::string(argv[1]) == "cross") return run_cross(argv);
    if (argc == 2 && std::string(argv[1]) == "configure") return run_configure();
    std::fprintf(stderr, "usage: see the head of cas_facade.cpp\n");
    return 2;
}
