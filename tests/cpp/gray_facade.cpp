// One-channel (GRAY / Y800) frames through the C++ facade, the plugin's asynchronous path:
//   FrameIngest::SelectY800 -> upload_obs_frame -> StabilizationFilter::apply(std::move(frame), frame) -> download_ocl_frame
// and WarpMesh::apply and the two lvk::remap launchers on an 8UC1 frame.
// usage: gray_facade <rows> <cols> <n frames> <delay> <clip.bin> <out.bin> <ops.bin>
//   clip.bin: n tight planes; out.bin: the emitted planes; ops.bin: frame 0 through WarpMesh::apply (3 x 3), remap(homography), remap(offset map), one after the other
#include <lvk/FrameIngest.hpp>
#include <lvk/WarpMesh.hpp>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "facade_util.hpp"

int main(int argc, char** argv)
{
    if (argc < 8) { std::fprintf(stderr, "usage\n"); return 2; }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), n = std::atoi(argv[3]), delay = std::atoi(argv[4]);
    const size_t frame_bytes = (size_t)rows * cols;
    std::vector<uint8_t> clip(frame_bytes * n), back(frame_bytes);
    if (!read_file(argv[5], clip)) return 2;
    FILE* out = std::fopen(argv[6], "wb");
    if (!out) return 2;
    if (lvk::FrameIngest::Select(LVK_VIDEO_FORMAT_Y800) != nullptr) { std::fprintf(stderr, "Select(Y800)\n"); return 1; }
    auto ingest = lvk::FrameIngest::SelectY800();
    if (!ingest || ingest->obs_format() != LVK_VIDEO_FORMAT_Y800 || ingest->ocl_format() != lvk::VideoFrame::GRAY) return 1;
    lvk::StabilizationFilter filter;
    filter.reconfigure([&](lvk::StabilizationFilterSettings& s) {
        s.detection_resolution = {480, 270}; s.detection_regions = {2, 1}; s.motion_resolution = {2, 2};
        s.acceptance_threshold = 3.0f; s.track_local_motions = false;
        s.max_feature_density = 0.12f; s.min_feature_density = 0.04f; s.accumulation_rate = 3.0f;
        s.corrective_limits = {0.05f, 0.05f}; s.crop_to_stable_region = true; s.background_colour = {105, 212, 235};
        s.predictive_samples = (size_t)delay; s.min_scene_quality = 0.3f; s.min_tracking_quality = 0.2f;
    });
    lvk::Frame frame, first;
    int emitted = 0;
    for (int k = 0; k < n; k++)
    {
        fake_obs_source_frame obs;
        obs.width = cols; obs.height = rows; obs.format = LVK_VIDEO_FORMAT_Y800; obs.timestamp = 500 + k;
        obs.data[0] = clip.data() + frame_bytes * k; obs.linesize[0] = cols;
        ingest->upload_obs_frame(&obs, frame);
        if (frame.format != lvk::VideoFrame::GRAY || frame.type() != CV_8UC1 || frame.channels() != 1 || (int)frame.step != cols) { std::fprintf(stderr, "not a GRAY frame\n"); return 1; }
        if (k == 0) first = frame.clone();
        filter.apply(std::move(frame), frame);
        if (frame.empty()) continue;
        if (frame.timestamp != (uint64_t)(500 + k - delay) || frame.format != lvk::VideoFrame::GRAY || frame.channels() != 1) { std::fprintf(stderr, "emitted frame\n"); return 1; }
        fake_obs_source_frame dst;
        dst.width = cols; dst.height = rows; dst.format = LVK_VIDEO_FORMAT_Y800;
        std::fill(back.begin(), back.end(), 0x5A);
        dst.data[0] = back.data(); dst.linesize[0] = cols;
        ingest->download_ocl_frame(frame, &dst);
        std::fwrite(back.data(), 1, back.size(), out);
        emitted++;
    }
    std::fclose(out);

    // the image operations on the 8UC1 frame
    FILE* ops = std::fopen(argv[7], "wb");
    if (!ops) return 2;
    auto dump = [&](const lvk::VideoFrame& f) {
        if (f.channels() != 1 || f.rows != rows || f.cols != cols || f.format != lvk::VideoFrame::GRAY) return false;
        f.download(back.data());
        return std::fwrite(back.data(), 1, back.size(), ops) == back.size();
    };
    lvk::WarpMesh mesh(cv::Size(3, 3));
    for (int i = 0; i < 18; i++) mesh.offsets()[i] = 0.01f * (float)((i * 7) % 5 - 2);
    lvk::VideoFrame warped;
    mesh.apply(first, warped, {77, 0, 0});
    if (!dump(warped)) { std::fprintf(stderr, "WarpMesh::apply\n"); return 1; }
    const double h[9] = {0.98, 0.05, 3.25, -0.04, 1.01, -2.5, 1e-5, 0.0, 1.0};
    lvk::VideoFrame byh; byh.format = lvk::VideoFrame::GRAY;
    lvk::remap(first, byh, lvk::Homography(h), {77, 0, 0}, true);
    if (!dump(byh)) { std::fprintf(stderr, "remap(homography)\n"); return 1; }
    std::vector<float> offs((size_t)rows * cols * 2);
    for (size_t i = 0; i + 1 < offs.size(); i += 2) { offs[i] = 1.37f; offs[i + 1] = -0.61f; }
    lvk::OffsetMap map;
    map.upload(offs.data(), cv::Size(cols, rows), first.context());
    lvk::VideoFrame bymap; bymap.format = lvk::VideoFrame::GRAY;
    lvk::remap(first, bymap, map, {77, 0, 0});
    if (!dump(bymap)) { std::fprintf(stderr, "remap(offset map)\n"); return 1; }
    std::fclose(ops);
    std::printf("stream ok: %d frames\n", emitted);
    return 0;
}
