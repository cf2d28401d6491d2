// lvk::HostFrameOBS + StabilizationFilter::apply(const HostFrameOBS&, HostFrameOBS&) of the C++ facade (include/lvk/LiveVisionKit.hpp): a stream of host
// frames of one OBS video format through lvk_hip_stab_push_obs_host, the way a host that owns pinned obs_source_frame planes would drive it.
// usage: obs_host_facade <obs format> <rows> <cols> <n frames> <delay> <planes.bin> <out.bin>
//   planes.bin = n frames' tight planes one after the other; out.bin = the emitted frames' planes, tight (for RGBA / BGRA / BGRX the rows * cols * 3
//   bytes the reference writes, then zeros: the last quarter of the plane is not the filter's).
#include <lvk/LiveVisionKit.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "facade_util.hpp"

int main(int argc, char** argv)
{
    if (argc < 8) { std::fprintf(stderr, "usage\n"); return 2; }
    const int fmt = std::atoi(argv[1]), rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), n = std::atoi(argv[4]), delay = std::atoi(argv[5]);
    int prow[3] = {0, 0, 0}, pbytes[3] = {0, 0, 0};
    const int np = lvk::HostFrameOBS::plane_table(fmt, rows, cols, prow, pbytes);
    if (np == 0 || lvk::HostFrameOBS::plane_table(LVK_VIDEO_FORMAT_Y800, rows, cols, prow, pbytes) != 0) { std::fprintf(stderr, "plane_table\n"); return 1; }
    lvk::HostFrameOBS::plane_table(fmt, rows, cols, prow, pbytes);
    size_t frame_bytes = 0;
    for (int i = 0; i < np; i++) frame_bytes += (size_t)prow[i] * pbytes[i];
    std::vector<uint8_t> clip(frame_bytes * n);
    if (!read_file(argv[6], clip)) return 2;
    FILE* out = std::fopen(argv[7], "wb");
    if (!out) return 2;
    const bool rgbx = fmt == LVK_VIDEO_FORMAT_RGBA || fmt == LVK_VIDEO_FORMAT_BGRA || fmt == LVK_VIDEO_FORMAT_BGRX;

    lvk::StabilizationFilter filter;
    filter.reconfigure([&](lvk::StabilizationFilterSettings& s) {
        s.detection_resolution = {480, 270}; s.detection_regions = {2, 1}; s.motion_resolution = {2, 2};
        s.acceptance_threshold = 3.0f; s.track_local_motions = false;
        s.max_feature_density = 0.12f; s.min_feature_density = 0.04f; s.accumulation_rate = 3.0f;
        s.corrective_limits = {0.05f, 0.05f}; s.crop_to_stable_region = true; s.background_colour = {105, 212, 235};
        s.predictive_samples = (size_t)delay; s.min_scene_quality = 0.3f; s.min_tracking_quality = 0.2f;
    });
    filter.set_overlap(true);
    lvk::HostFrameOBS in[2], result;
    int emitted = 0;
    for (int k = 0; k < n; k++)
    {
        lvk::HostFrameOBS& f = in[k & 1];
        f.create({cols, rows}, fmt);
        if (f.bytes() != frame_bytes || f.data[0] == nullptr || f.linesize[0] != pbytes[0]) { std::fprintf(stderr, "layout\n"); return 1; }
        std::memcpy(f.data[0], clip.data() + frame_bytes * k, frame_bytes);         // (one block: the planes lie one after the other)
        f.timestamp = 500 + k;
        filter.apply(f, result);
        std::memset(f.data[0], 0x33, frame_bytes);                                    // consumed on return: wiping the input must not matter
        if (result.empty()) continue;
        result.wait();
        if (result.timestamp != (uint64_t)(500 + k - delay) || result.format != fmt || result.rows != rows || result.cols != cols) { std::fprintf(stderr, "metadata\n"); return 1; }
        std::vector<uint8_t> back(frame_bytes, 0);
        std::memcpy(back.data(), result.data[0], rgbx ? (size_t)rows * cols * 3 : frame_bytes);
        std::fwrite(back.data(), 1, back.size(), out);
        emitted++;
    }
    std::fclose(out);
    std::printf("stream ok: %d frames\n", emitted);
    return 0;
}
