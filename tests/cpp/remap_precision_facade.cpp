// lvk::RemapPrecision through the C++ facade: StabilizationFilter::set_remap_precision / remap_precision() and hip::Context::set_remap_precision, which
// WarpMesh::apply on that context follows.
// usage: remap_precision_facade <rows> <cols> <n frames> <delay> <clip.bin> <out.bin>
//   clip.bin: n tight packed YUV frames; out.bin: for Exact, then for OneLSB: the first three emitted frames, then frame 0 through WarpMesh::apply (5 x 5)
#include <lvk/LiveVisionKit.hpp>
#include <lvk/WarpMesh.hpp>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "facade_util.hpp"

int main(int argc, char** argv)
{
    if (argc < 7) { std::fprintf(stderr, "usage\n"); return 2; }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), n = std::atoi(argv[3]), delay = std::atoi(argv[4]);
    const size_t frame_bytes = (size_t)rows * cols * 3;
    std::vector<uint8_t> clip(frame_bytes * n), back(frame_bytes);
    if (!read_file(argv[5], clip)) return 2;
    FILE* out = std::fopen(argv[6], "wb");
    if (!out) return 2;
    for (const lvk::RemapPrecision precision : {lvk::RemapPrecision::Exact, lvk::RemapPrecision::OneLSB})
    {
        lvk::StabilizationFilter filter;
        filter.reconfigure([&](lvk::StabilizationFilterSettings& s) {
            s.detection_resolution = {480, 270}; s.detection_regions = {2, 1}; s.motion_resolution = {2, 2};
            s.acceptance_threshold = 3.0f; s.track_local_motions = false;
            s.max_feature_density = 0.12f; s.min_feature_density = 0.04f; s.accumulation_rate = 3.0f;
            s.corrective_limits = {0.05f, 0.05f}; s.crop_to_stable_region = true; s.background_colour = {105, 212, 235};
            s.predictive_samples = (size_t)delay; s.min_scene_quality = 0.3f; s.min_tracking_quality = 0.2f;
        });
        if (filter.remap_precision() != lvk::RemapPrecision::Exact) { std::fprintf(stderr, "a filter is created Exact\n"); return 1; }
        filter.set_remap_precision(precision);
        if (filter.remap_precision() != precision) { std::fprintf(stderr, "remap_precision()\n"); return 1; }
        if (filter.context()->remap_precision() != lvk::RemapPrecision::Exact) { std::fprintf(stderr, "the filter's setting leaked into its context\n"); return 1; }
        int emitted = 0;
        lvk::VideoFrame first;
        for (int k = 0; k < n && emitted < 3; k++)
        {
            lvk::VideoFrame frame;
            frame.upload(clip.data() + frame_bytes * k, rows, cols, lvk::VideoFrame::YUV, (uint64_t)k, filter.context());
            if (k == 0) first = frame.clone();
            lvk::VideoFrame result;
            filter.apply(std::move(frame), result);
            if (result.empty()) continue;
            if (result.timestamp != (uint64_t)(k - delay)) { std::fprintf(stderr, "timestamp\n"); return 1; }
            result.download(back.data());
            std::fwrite(back.data(), 1, back.size(), out);
            emitted++;
        }
        if (emitted != 3) { std::fprintf(stderr, "emitted %d frames\n", emitted); return 1; }

        // the stateless route: the context's own setting
        first.context()->set_remap_precision(precision);
        if (first.context()->remap_precision() != precision) { std::fprintf(stderr, "Context::remap_precision()\n"); return 1; }
        lvk::WarpMesh mesh(cv::Size(5, 5));
        for (int i = 0; i < 50; i++) mesh.offsets()[i] = 0.01f * (float)((i * 7) % 5 - 2);
        lvk::VideoFrame warped;
        mesh.apply(first, warped, {16, 128, 128});
        first.context()->set_remap_precision(lvk::RemapPrecision::Exact);
        if (warped.rows != rows || warped.cols != cols) { std::fprintf(stderr, "WarpMesh::apply\n"); return 1; }
        warped.download(back.data());
        std::fwrite(back.data(), 1, back.size(), out);
    }
    std::fclose(out);
    std::printf("precision facade ok\n");
    return 0;
}
