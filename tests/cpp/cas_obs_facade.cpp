// lvk::CASFilter::apply(VideoFrame420, VideoFrame420) and apply(VideoFrameOBS, VideoFrameOBS) of the C++ facade (include/lvk/CASFilter.hpp): the planes
// of an I420 / NV12 frame (lvk_hip_cas_yuv420) or of any OBS video format (lvk_hip_cas_obs) through the CAS filter in one call.
//
// cas_obs_facade 420 <nv12> <rows> <cols> <sharpness> <in.bin> <out.bin>
// cas_obs_facade obs <video format number> <rows> <cols> <sharpness> <in.bin> <out.bin>
//   in.bin / out.bin: the planes of the frame one after the other, tightly packed.  The output block is filled with 0x5A before the first call, so that
//   bytes the egress leaves alone come back as that.  Applies twice -- into the prepared output and again into it --, checks size, layout or format,
//   timestamp, context and that the input planes are untouched, then the filter's assertions: a refused call throws through the assert handler and
//   leaves the output as it was.
#include <lvk/LiveVisionKit.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "facade_util.hpp"

namespace {

bool same_layout(const lvk::VideoFrame420& a, const lvk::VideoFrame420& b) { return a.nv12 == b.nv12; }
bool same_layout(const lvk::VideoFrameOBS& a, const lvk::VideoFrameOBS& b) { return a.format == b.format; }
const uint8_t* base(const lvk::VideoFrame420& f) { return f.y(); }
const uint8_t* base(const lvk::VideoFrameOBS& f) { return f.data[0]; }
size_t bytes_of(const lvk::VideoFrame420& f) { return (size_t)f.cols * f.rows * 3 / 2; }
size_t bytes_of(const lvk::VideoFrameOBS& f) { return f.bytes(); }

template <class Frame, class Layout>
int run(Layout layout, int rows, int cols, float sharpness, const char* in_path, const char* out_path)
{
    Frame input, output;
    input.create({cols, rows}, layout);
    std::vector<uint8_t> host(bytes_of(input)), back(host.size());
    if (!read_file(in_path, host)) return 2;
    input.upload(host.data(), rows, cols, layout, 41);
    std::vector<uint8_t> first(host.size(), 0x5A), second(first.size());
    output.upload(first.data(), rows, cols, layout, 0, input.context());
    const uint8_t* kept = base(output);

    lvk::CASFilterSettings settings;
    settings.sharpness = sharpness;
    lvk::CASFilter filter(settings);
    filter.apply(input, output, true);
    if (output.empty() || output.rows != rows || output.cols != cols || !same_layout(output, input) || output.timestamp != 41) return 1;
    if (base(output) != kept || base(output) == base(input) || output.context() != input.context()) return 1;   // the output of the right size is written, not replaced
    output.download(first.data());
    input.timestamp = 42;
    filter.apply(input, output);
    if (base(output) != kept || output.timestamp != 42) return 1;
    output.download(second.data());
    if (second != first) return 1;
    input.download(back.data());
    if (back != host) return 1;                               // out of place: the input planes are as they were
    if (!(filter.timings().average().seconds() > 0.0)) return 1;
    if (!write_file(out_path, first)) return 2;

    // a fresh output is created at the input's size, layout and context
    {
        Frame made;
        filter.apply(input, made);
        if (made.empty() || made.rows != rows || made.cols != cols || !same_layout(made, input) || made.context() != input.context() || made.timestamp != 42) return 1;
    }

    // refused like the reference's asserts: the input as its own output, an empty input, a sharpness outside [0, 1]
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0, expected = 0;
    try { filter.apply(input, input); } catch (const std::runtime_error&) { refused++; }
    expected++;
    {
        Frame none, out;
        try { filter.apply(none, out); } catch (const std::runtime_error&) { refused += out.empty() ? 1 : 0; }
        expected++;
    }
    {
        lvk::CASFilterSettings bad;
        bad.sharpness = 1.5f;
        try { filter.configure(bad); } catch (const std::runtime_error&) { refused += filter.settings().sharpness == sharpness ? 1 : 0; }
        expected++;
    }
    input.download(back.data());
    output.download(second.data());
    if (refused != expected || back != host || second != first) { std::fprintf(stderr, "%d of %d refused\n", refused, expected); return 1; }
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 8) { std::fprintf(stderr, "usage: see the head of cas_obs_facade.cpp\n"); return 2; }
    const bool planes420 = std::strcmp(argv[1], "420") == 0;
    const int layout = std::atoi(argv[2]), rows = std::atoi(argv[3]), cols = std::atoi(argv[4]);
    const float sharpness = (float)std::atof(argv[5]);
    const int rc = planes420 ? run<lvk::VideoFrame420, bool>(layout != 0, rows, cols, sharpness, argv[6], argv[7])
                             : run<lvk::VideoFrameOBS, int>(layout, rows, cols, sharpness, argv[6], argv[7]);
    if (rc == 0) std::printf("cas %s ok: %d %dx%d\n", planes420 ? "420" : "obs", layout, cols, rows);
    return rc;
}
