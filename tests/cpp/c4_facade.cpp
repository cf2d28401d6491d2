// Four-channel (BGRA / RGBA) frames through the C++ facade, the plugin's asynchronous path:
//   FrameIngest::SelectRGBX -> upload_obs_frame -> StabilizationFilter::apply(std::move(frame), frame) -> download_ocl_frame
// and WarpMesh::apply and the two lvk::remap launchers on an 8UC4 frame.
// usage: c4_facade <rows> <cols> <n frames> <delay> <video format> <clip.bin> <out.bin> <ops.bin>
//   video format: LVK_VIDEO_FORMAT_BGRA / _BGRX / _RGBA; clip.bin: n frames of rows x cols x 4 bytes, rows `pad` bytes apart (see below); out.bin: the emitted
//   frames, tight; ops.bin: frame 0 through WarpMesh::apply (3 x 3), remap(homography), remap(offset map), one after the other
#include <lvk/FrameIngest.hpp>
#include <lvk/WarpMesh.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "facade_util.hpp"

int main(int argc, char** argv)
{
    if (argc < 9) { std::fprintf(stderr, "usage\n"); return 2; }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), n = std::atoi(argv[3]), delay = std::atoi(argv[4]), vf = std::atoi(argv[5]);
    const size_t row = (size_t)4 * cols, frame_bytes = row * rows;
    const size_t host_step = row + 8;                          // the OBS frame's linesize is not the row: both transfers honour it
    std::vector<uint8_t> clip(frame_bytes * n), pitched(host_step * rows), back(host_step * rows), tight(frame_bytes);
    if (!read_file(argv[6], clip)) return 2;
    FILE* out = std::fopen(argv[7], "wb");
    if (!out) return 2;
    const lvk::VideoFrame::Format fmt = vf == LVK_VIDEO_FORMAT_RGBA ? lvk::VideoFrame::RGBA : lvk::VideoFrame::BGRA;
    // Select keeps its answer for these formats: DirectIngest's three-channel frame
    auto direct = lvk::FrameIngest::Select(vf);
    if (!direct || lvk::VideoFrame::channels_of(direct->ocl_format()) != 3) { std::fprintf(stderr, "Select changed its answer\n"); return 1; }
    if (lvk::FrameIngest::SelectRGBX(LVK_VIDEO_FORMAT_BGR3) != nullptr || lvk::FrameIngest::SelectRGBX(LVK_VIDEO_FORMAT_I420) != nullptr) { std::fprintf(stderr, "SelectRGBX(other)\n"); return 1; }
    auto ingest = lvk::FrameIngest::SelectRGBX(vf);
    if (!ingest || ingest->obs_format() != vf || ingest->ocl_format() != fmt) return 1;
    lvk::StabilizationFilter filter;
    filter.reconfigure([&](lvk::StabilizationFilterSettings& s) {
        s.detection_resolution = {480, 270}; s.detection_regions = {2, 1}; s.motion_resolution = {2, 2};
        s.acceptance_threshold = 3.0f; s.track_local_motions = false;
        s.max_feature_density = 0.12f; s.min_feature_density = 0.04f; s.accumulation_rate = 3.0f;
        s.corrective_limits = {0.05f, 0.05f}; s.crop_to_stable_region = true; s.background_colour = {105, 212, 235, 66};
        s.predictive_samples = (size_t)delay; s.min_scene_quality = 0.3f; s.min_tracking_quality = 0.2f;
    });
    lvk::Frame frame, first;
    int emitted = 0;
    for (int k = 0; k < n; k++)
    {
        for (int r = 0; r < rows; r++) std::memcpy(pitched.data() + host_step * r, clip.data() + frame_bytes * k + row * r, row);
        fake_obs_source_frame obs;
        obs.width = cols; obs.height = rows; obs.format = vf; obs.timestamp = 500 + k;
        obs.data[0] = pitched.data(); obs.linesize[0] = (uint32_t)host_step;
        ingest->upload_obs_frame(&obs, frame);
        if (frame.format != fmt || frame.type() != CV_8UC4 || frame.channels() != 4 || frame.step < row) { std::fprintf(stderr, "not a four-channel frame\n"); return 1; }
        if (k == 0) first = frame.clone();
        filter.apply(std::move(frame), frame);
        if (frame.empty()) continue;
        if (frame.timestamp != (uint64_t)(500 + k - delay) || frame.format != fmt || frame.channels() != 4) { std::fprintf(stderr, "emitted frame\n"); return 1; }
        fake_obs_source_frame dst;
        dst.width = cols; dst.height = rows; dst.format = vf;
        std::fill(back.begin(), back.end(), 0x5A);
        dst.data[0] = back.data(); dst.linesize[0] = (uint32_t)host_step;
        ingest->download_ocl_frame(frame, &dst);
        for (int r = 0; r < rows; r++)
        {
            for (size_t b = row; b < host_step; b++) if (back[host_step * r + b] != 0x5A) { std::fprintf(stderr, "download wrote past the row\n"); return 1; }
            std::memcpy(tight.data() + row * r, back.data() + host_step * r, row);
        }
        std::fwrite(tight.data(), 1, tight.size(), out);
        emitted++;
    }
    std::fclose(out);

    // the image operations on the 8UC4 frame: all four background values are used
    FILE* ops = std::fopen(argv[8], "wb");
    if (!ops) return 2;
    auto dump = [&](const lvk::VideoFrame& f) {
        if (f.channels() != 4 || f.rows != rows || f.cols != cols || f.format != fmt) return false;
        f.download(tight.data());
        return std::fwrite(tight.data(), 1, tight.size(), ops) == tight.size();
    };
    const cv::Scalar bg(77, 201, 5, 130);
    lvk::WarpMesh mesh(cv::Size(3, 3));
    for (int i = 0; i < 18; i++) mesh.offsets()[i] = 0.01f * (float)((i * 7) % 5 - 2);
    lvk::VideoFrame warped;
    mesh.apply(first, warped, bg);
    if (!dump(warped)) { std::fprintf(stderr, "WarpMesh::apply\n"); return 1; }
    const double h[9] = {0.98, 0.05, 3.25, -0.04, 1.01, -2.5, 1e-5, 0.0, 1.0};
    lvk::VideoFrame byh; byh.format = fmt;
    lvk::remap(first, byh, lvk::Homography(h), bg, true);
    if (!dump(byh)) { std::fprintf(stderr, "remap(homography)\n"); return 1; }
    std::vector<float> offs((size_t)rows * cols * 2);
    for (size_t i = 0; i + 1 < offs.size(); i += 2) { offs[i] = 1.37f; offs[i + 1] = -0.61f; }
    lvk::OffsetMap map;
    map.upload(offs.data(), cv::Size(cols, rows), first.context());
    lvk::VideoFrame bymap; bymap.format = fmt;
    lvk::remap(first, bymap, map, bg);
    if (!dump(bymap)) { std::fprintf(stderr, "remap(offset map)\n"); return 1; }
    std::fclose(ops);
    std::printf("stream ok: %d frames\n", emitted);
    return 0;
}
