// lvk::FSRFilter::apply(VideoFrame420, VideoFrame420) and apply(VideoFrameOBS, VideoFrameOBS) of the C++ facade (include/lvk/FSRFilter.hpp): the planes
// of an I420 / NV12 frame (lvk_hip_fsr_yuv420) or of any OBS video format (lvk_hip_fsr_obs) through the FSR filter in one call.
//
// fsr_obs_facade 420 <nv12> <rows> <cols> <out_rows> <out_cols> <multiplier> <left> <top> <right> <bottom> <sharpness> <in.bin> <out.bin>
// fsr_obs_facade obs <video format number> ... the same
//   multiplier > 0: the settings are the multiplier alone (the output size follows the frame); otherwise the explicit output size out_cols x out_rows
//   without the aspect-ratio fit.  left .. bottom: the crops.  out_rows x out_cols is what the settings must produce.  sharpness >= 0 (obs only): the
//   chain FSRFilter -> CASFilter, out.bin holds the sharpened planes.
//   in.bin / out.bin: the planes of the frame one after the other, tightly packed.  The output block is filled with 0x5A before the first call, so that
//   bytes the egress leaves alone come back as that.  Applies twice -- into the prepared output and again into it --, checks size, layout or format,
//   timestamp, context and that the input planes are untouched, then the skip path and the filter's assertions: a refused call throws through the
//   assert handler and leaves the output as it was.
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
bool even_cols_only(const lvk::VideoFrame420&) { return true; }
bool even_cols_only(const lvk::VideoFrameOBS& f)
{
    return f.format == LVK_VIDEO_FORMAT_I420 || f.format == LVK_VIDEO_FORMAT_I40A || f.format == LVK_VIDEO_FORMAT_NV12 || f.format == LVK_VIDEO_FORMAT_I422
           || f.format == LVK_VIDEO_FORMAT_I42A || f.format == LVK_VIDEO_FORMAT_YUY2 || f.format == LVK_VIDEO_FORMAT_YVYU || f.format == LVK_VIDEO_FORMAT_UYVY;
}

// the sharpening stage of the chain: on VideoFrameOBS only
bool sharpen(const lvk::VideoFrame420&, float, std::vector<uint8_t>&) { return false; }
bool sharpen(const lvk::VideoFrameOBS& scaled, float sharpness, std::vector<uint8_t>& planes)
{
    lvk::CASFilterSettings settings;
    settings.sharpness = sharpness;
    lvk::CASFilter cas(settings);
    lvk::VideoFrameOBS sharp;
    planes.assign(scaled.bytes(), 0x5A);
    sharp.upload(planes.data(), scaled.rows, scaled.cols, scaled.format, 0, scaled.context());
    cas.apply(scaled, sharp);
    if (sharp.rows != scaled.rows || sharp.cols != scaled.cols || sharp.format != scaled.format || sharp.timestamp != scaled.timestamp) return false;
    sharp.download(planes.data());
    return true;
}

struct Args { int rows, cols, out_rows, out_cols; float multiplier; int crop[4]; float sharpness; const char *in_path, *out_path; };

template <class Frame, class Layout>
int run(Layout layout, const Args& a)
{
    Frame input, output;
    input.create({a.cols, a.rows}, layout);
    std::vector<uint8_t> host(bytes_of(input)), back(host.size());
    if (!read_file(a.in_path, host)) return 2;
    input.upload(host.data(), a.rows, a.cols, layout, 41);
    output.create({a.out_cols, a.out_rows}, layout, input.context());
    std::vector<uint8_t> first(bytes_of(output), 0x5A), second(first.size());
    output.upload(first.data(), a.out_rows, a.out_cols, layout, 0, input.context());
    const uint8_t* kept = base(output);

    lvk::FSRFilterSettings settings;
    if (a.multiplier > 0.0f) settings.size_multiplier = a.multiplier;
    else { settings.output_size = {a.out_cols, a.out_rows}; settings.maintain_aspect_ratio = false; }
    settings.crop_left = a.crop[0]; settings.crop_top = a.crop[1]; settings.crop_right = a.crop[2]; settings.crop_bottom = a.crop[3];
    lvk::FSRFilter filter(settings);
    filter.apply(input, output, true);
    if (output.empty() || output.rows != a.out_rows || output.cols != a.out_cols || !same_layout(output, input) || output.timestamp != 41) return 1;
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
    std::vector<uint8_t> result = first;
    if (a.sharpness >= 0.0f && !sharpen(output, a.sharpness, result)) return 1;
    if (!write_file(a.out_path, result)) return 2;

    // a fresh output is created at the output size in the input's layout and context
    {
        Frame made;
        filter.apply(input, made);
        if (made.empty() || made.rows != a.out_rows || made.cols != a.out_cols || !same_layout(made, input) || made.context() != input.context()
            || made.timestamp != 42) return 1;
    }
    // the skip path: 1 : 1 on the whole frame goes through unchanged, as the frame itself
    {
        lvk::FSRFilter same;
        Frame through;
        same.apply(input, through);
        if (through.empty() || base(through) != base(input) || through.rows != a.rows || through.cols != a.cols || !same_layout(through, input)
            || through.timestamp != 42) return 1;
    }

    // refused like the reference's asserts: the input as its own output, an empty input, an output size whose parity the format does not take
    lvk::context::assert_handler = [](std::string, std::string, std::string assertion) { throw std::runtime_error(assertion); };
    int refused = 0, expected = 0;
    try { filter.apply(input, input); } catch (const std::runtime_error&) { refused++; }
    expected++;
    {
        Frame none, out;
        try { filter.apply(none, out); } catch (const std::runtime_error&) { refused += out.empty() ? 1 : 0; }
        expected++;
    }
    if (even_cols_only(input))
    {
        lvk::FSRFilterSettings odd;
        odd.output_size = {a.out_cols + 1, a.out_rows};
        odd.maintain_aspect_ratio = false;
        lvk::FSRFilter bad(odd);
        const std::string size = std::to_string(a.out_cols + 1) + " x " + std::to_string(a.out_rows);
        try { bad.apply(input, output); }
        catch (const std::runtime_error& e) { refused += std::string(e.what()).find(size) != std::string::npos ? 1 : 0; }      // the message names the size
        expected++;
    }
    input.download(back.data());
    output.download(second.data());
    if (refused != expected || back != host || second != first || base(output) != kept) { std::fprintf(stderr, "%d of %d refused\n", refused, expected); return 1; }
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 15) { std::fprintf(stderr, "usage: see the head of fsr_obs_facade.cpp\n"); return 2; }
    const bool planes420 = std::strcmp(argv[1], "420") == 0;
    const int layout = std::atoi(argv[2]);
    const Args a{std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), (float)std::atof(argv[7]),
                 {std::atoi(argv[8]), std::atoi(argv[9]), std::atoi(argv[10]), std::atoi(argv[11])}, (float)std::atof(argv[12]), argv[13], argv[14]};
    const int rc = planes420 ? run<lvk::VideoFrame420, bool>(layout != 0, a) : run<lvk::VideoFrameOBS, int>(layout, a);
    if (rc == 0) std::printf("fsr %s ok: %d %dx%d -> %dx%d\n", planes420 ? "420" : "obs", layout, a.cols, a.rows, a.out_cols, a.out_rows);
    return rc;
}
