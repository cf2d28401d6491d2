// lvk::DeblockingFilter of the C++ facade (include/lvk/DeblockingFilter.hpp) driven the way its two users drive the reference's.
//
// deblocking_facade apply <format> <rows> <cols> <levels> <block> <k> <scaling> <frame.bin> <out prefix>
//   the ADB filter's test mode (Modules/OBS-Plugin/Sources/Enhancement/ADBFilter.cpp:130-136): apply(frame, frame, true), then
//   draw_influence(frame); writes <prefix>.apply and <prefix>.influence (the frame after each) and prints the filter region.
// deblocking_facade --stream <obs format> <rows> <cols> <n frames> <delay> <with stabilizer> <planes.bin> <out.bin>
//   the plugin's asynchronous path (Interop/VisionFilter.cpp:151-253): upload_obs_frame -> filter.apply(std::move(frame), frame) ->
//   download_ocl_frame, where the filter is a DeblockingFilter or, as the editor chains them (Modules/VideoEditor/VideoIOConfiguration.cpp:
//   437-446), CompositeFilter{StabilizationFilter, DeblockingFilter}; out.bin = the emitted frames' tight planes.
#include <lvk/LiveVisionKit.hpp>
#include <lvk/FrameIngest.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "facade_util.hpp"

static int run_apply(char** argv)
{
    const int fmt = std::atoi(argv[2]), rows = std::atoi(argv[3]), cols = std::atoi(argv[4]);
    lvk::DeblockingFilterSettings s;
    s.detection_levels = (uint32_t)std::atoi(argv[5]); s.block_size = (uint32_t)std::atoi(argv[6]);
    s.filter_size = (uint32_t)std::atoi(argv[7]); s.filter_scaling = (float)std::atof(argv[8]);
    std::vector<uint8_t> host((size_t)rows * cols * 3);
    if (!read_file(argv[9], host)) return 2;
    const std::string prefix = argv[10];

    lvk::DeblockingFilter filter(s);
    lvk::Frame frame;
    frame.upload(host.data(), rows, cols, (lvk::VideoFrame::Format)fmt, 7);
    filter.apply(frame, frame, true);
    if (frame.timestamp != 7 || frame.rows != rows || frame.cols != cols) return 1;
    frame.download(host.data());
    if (!write_file(prefix + ".apply", host)) return 2;
    filter.draw_influence(frame);
    frame.download(host.data());
    if (!write_file(prefix + ".influence", host)) return 2;
    const cv::Rect r = filter.filter_region();
    std::printf("apply ok: region %d %d %d %d\n", r.x, r.y, r.width, r.height);
    return 0;
}

static int run_stream(char** argv)
{
    const int fmt = std::atoi(argv[2]), rows = std::atoi(argv[3]), cols = std::atoi(argv[4]), n = std::atoi(argv[5]), delay = std::atoi(argv[6]);
    const bool with_stab = std::atoi(argv[7]) != 0;
    if (fmt != 1) return 2;                                  // I420
    const size_t ybytes = (size_t)rows * cols, cbytes = (size_t)(rows / 2) * (cols / 2), frame_bytes = ybytes + 2 * cbytes;
    std::vector<uint8_t> clip(frame_bytes * n), back(frame_bytes);
    if (!read_file(argv[8], clip)) return 2;
    FILE* out = std::fopen(argv[9], "wb");
    if (!out) return 2;
    auto ingest = lvk::FrameIngest::Select(fmt);
    if (!ingest) return 1;

    auto deblocker = std::make_shared<lvk::DeblockingFilter>();
    std::shared_ptr<lvk::VideoFilter> filter = deblocker;
    if (with_stab)
    {
        auto stab = std::make_shared<lvk::StabilizationFilter>();
        stab->reconfigure([&](lvk::StabilizationFilterSettings& s) {
            s.detection_resolution = {480, 270}; s.detection_regions = {2, 1}; s.motion_resolution = {2, 2};
            s.acceptance_threshold = 3.0f; s.track_local_motions = false;
            s.max_feature_density = 0.12f; s.min_feature_density = 0.04f; s.accumulation_rate = 3.0f;
            s.corrective_limits = {0.05f, 0.05f}; s.crop_to_stable_region = true; s.background_colour = {105, 212, 235};
            s.predictive_samples = (size_t)delay; s.min_scene_quality = 0.3f; s.min_tracking_quality = 0.2f;
        });
        filter = std::make_shared<lvk::CompositeFilter>(std::initializer_list<std::shared_ptr<lvk::VideoFilter>>{stab, deblocker});
    }
    lvk::Frame frame;
    int emitted = 0;
    for (int k = 0; k < n; k++)
    {
        fake_obs_source_frame obs;
        obs.width = cols; obs.height = rows; obs.format = fmt; obs.timestamp = 500 + k;
        uint8_t* p = clip.data() + frame_bytes * k;
        obs.data[0] = p; obs.linesize[0] = cols;
        obs.data[1] = p + ybytes; obs.linesize[1] = cols / 2;
        obs.data[2] = p + ybytes + cbytes; obs.linesize[2] = cols / 2;
        ingest->upload_obs_frame(&obs, frame);
        filter->apply(std::move(frame), frame);
        if (frame.empty()) continue;
        fake_obs_source_frame dst;
        dst.width = cols; dst.height = rows; dst.format = fmt;
        std::fill(back.begin(), back.end(), 0x5A);
        dst.data[0] = back.data(); dst.linesize[0] = cols;
        dst.data[1] = back.data() + ybytes; dst.linesize[1] = cols / 2;
        dst.data[2] = back.data() + ybytes + cbytes; dst.linesize[2] = cols / 2;
        ingest->download_ocl_frame(frame, &dst);
        std::fwrite(back.data(), 1, back.size(), out);
        emitted++;
    }
    std::fclose(out);
    const cv::Rect r = deblocker->filter_region();
    std::printf("stream ok: %d frames, region %d %d %d %d\n", emitted, r.x, r.y, r.width, r.height);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 11 && std::string(argv[1]) == "apply") return run_apply(argv);
    if (argc == 10 && std::string(argv[1]) == "--stream") return run_stream(argv);
    std::fprintf(stderr, "usage: see the head of deblocking_facade.cpp\n");
    return 2;
}
