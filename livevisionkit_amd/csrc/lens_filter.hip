// lvk::LCFilter, the OBS plugin's lens-correction filter (Modules/OBS-Plugin/Sources/Enhancement/LCFilter.cpp:133-192), as an object of the C-ABI
// (lvk_hip_lens_*) and the one kernel family it adds: k_remap_map_420, the materialised-map remap with the 4:2:0 egress in its sink
// (lvk_hip_remap_map_yuv420), the counterpart of k_remap_mesh_420 for MapCoord.  Everything the kernel is made of is in remap_core.hpp: remap_strip<true, W>
// with MapCoord and Sink420<NV12>, defined through LVK_REMAP_KERNEL so that the exact kernel and its 1-LSB twin share one body.
//
// The object owns what the plugin's filter owns: the camera profile, the offset map of the last frame size (lvk_lens_build_offsets of lens.hip, rebuilt
// when the size or the profile changed) and the test-mode grid, which is drawn BEFORE the warp so that it is warped with the frame.
#include "remap_core.hpp"
#include "yuv420_core.hpp"

using namespace yuv420;

namespace {

// Full grid only: a materialised map has no persistent-grid form (lvk_launch_remap_map)
LVK_REMAP_KERNEL(bool NV12, , k_remap_map_420,
                 (const uint8_t* __restrict__ src, int src_step, int rows, int cols, PlanesOut o, const uint8_t* __restrict__ map, int map_step, uint32_t bg),
{
    const MapCoord coord{map, map_step};
    remap_strip<true, W>(src, src_step, rows, cols, sink420<NV12>(o), rows, cols, coord, bg);
})

// the one launch of the family: every argument has been checked
int launch_remap_map_420(lvk_hip_ctx* ctx, const void* d_src, int src_step, const PlaneSet& dst, const void* d_map, int map_step, const uint8_t bg[3])
{
    launch_remap(ctx, LVK_REMAP_FORMS(k_remap_map_420, false, true), dst.nv12 != 0, dst.rows, dst.cols, RemapLaunch{ctx->stream, ctx->remap_precision}, 0,
                 (const uint8_t*)d_src, src_step, dst.rows, dst.cols, dst.out(), (const uint8_t*)d_map, map_step, pack_bg(bg));
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// col::MAGENTA[format] (Functions/Drawing.hpp) and the grid of LCFilter.cpp:182
constexpr uint8_t kMagentaYUV[3] = {105, 212, 234}, kMagentaBGR[3] = {255, 0, 255};
constexpr int kGridW = 32, kGridH = 32;
constexpr uint8_t kBackground[4] = {0, 0, 0, 0};              // WarpMesh::apply's default

} // namespace

struct lvk_hip_lens
{
    lvk_hip_ctx* ctx = nullptr;
    bool selected = false;                  // m_ProfileSelected
    lvk_camera_params profile{};
    int test_mode = 0;
    void* d_map = nullptr;                  // rows x cols float2, tightly packed; one map, of the last frame size
    int map_rows = 0, map_cols = 0;
    bool outdated = true;                   // m_MeshOutdated

    // prepare_undistort_maps (LCFilter.cpp:133-171): `m_MeshOutdated || size != frame.size()`.  The old map may still be read by a kernel on the stream:
    // its release waits for the stream, as lvk_hip_lens_map_destroy does.  rows, cols > 1.
    int prepare(int rows, int cols)
    {
        if (d_map && !outdated && rows == map_rows && cols == map_cols) return LVK_HIP_OK;
        std::vector<float> off; int view[4];
        lvk_lens_build_offsets(profile, rows, cols, off, view);
        void* d = nullptr;
        LVK_HIP_CHECK(ctx, hipMalloc(&d, off.size() * sizeof(float)));
        const hipError_t e = hipMemcpy(d, off.data(), off.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d); return ctx->fail(LVK_HIP_ERR_RUNTIME, hipGetErrorString(e)); }
        release_map();
        d_map = d; map_rows = rows; map_cols = cols; outdated = false;
        return LVK_HIP_OK;
    }
    void release_map()
    {
        if (!d_map) return;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_map);
        d_map = nullptr; map_rows = map_cols = 0;
    }
    int map_step() const { return map_cols * 8; }
};

namespace {

// the common head of the packed applies: a well-formed out-of-place pair of BPP-byte frames; with a profile the map needs more than one row and column
int packed_pair_ok(lvk_hip_lens* lens, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step, int bpp)
{
    lvk_hip_ctx* ctx = lens->ctx;
    LVK_HIP_REQUIRE(ctx, remap_plane_ok(d_src, src_step, rows, cols, bpp) && remap_plane_ok(d_dst, dst_step, rows, cols, bpp));
    LVK_HIP_REQUIRE(ctx, !lens->selected || (rows > 1 && cols > 1));
    LVK_HIP_REQUIRE(ctx, !lvk_pitched_overlap(d_src, src_step, rows, (long long)bpp * cols, d_dst, dst_step, rows, (long long)bpp * cols));
    return LVK_HIP_OK;
}

int copy_frame(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step, int bpp)
{
    LVK_HIP_CHECK(ctx, hipMemcpy2DAsync(d_dst, (size_t)dst_step, d_src, (size_t)src_step, (size_t)bpp * (size_t)cols, (size_t)rows, hipMemcpyDeviceToDevice, ctx->stream));
    return LVK_HIP_OK;
}

} // namespace

extern "C" {

int lvk_hip_remap_map_yuv420(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                             void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int nv12,
                             const void* d_map, int map_step, const uint8_t bg[3])
{
    LVK_HIP_ENTRY(ctx);
    const char* name = "lvk_hip_remap_map_yuv420";
    LVK_HIP_REQUIRE(ctx, remap_precision_known(ctx->remap_precision));
    LVK_HIP_REQUIRE(ctx, bg != nullptr);
    const PlaneSet dst = plane_set(o_y, oy_step, o_u, ou_step, o_v, ov_step, nv12, rows, cols);
    LVK_HIP_REQUIRE(ctx, well_formed(dst, true));
    LVK_HIP_REQUIRE(ctx, remap_plane_ok(d_src, src_step, rows, cols, 3) && remap_map_ok(d_map, map_step, rows, cols));
    const Span in[2] = {span_of(d_src, src_step, rows, 3 * cols), span_of(d_map, map_step, rows, 8 * cols)};
    const int rc = require_out_of_place(ctx, name, in, 2, dst);
    if (rc != LVK_HIP_OK) return rc;
    return launch_remap_map_420(ctx, d_src, src_step, dst, d_map, map_step, bg);
}

int lvk_hip_lens_configure(lvk_hip_lens* lens, const lvk_camera_params* profile, int test_mode)
{
    if (!lens) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = lens->ctx;
    // a profile lvk_lens_model_build refuses leaves the object as it was
    if (profile && (profile->fx == 0.0 || profile->fy == 0.0)) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_lens_configure: invalid camera profile (fx or fy is 0)");
    if (profile)
    {
        // LCFilter::configure (LCFilter.cpp:104-113): another profile makes the mesh outdated
        if (!lens->selected || std::memcmp(&lens->profile, profile, sizeof(*profile)) != 0) lens->outdated = true;
        lens->profile = *profile;
    }
    lens->selected = profile != nullptr;
    lens->test_mode = test_mode != 0;
    return LVK_HIP_OK;
}

int lvk_hip_lens_create(lvk_hip_ctx* ctx, const lvk_camera_params* profile, int test_mode, lvk_hip_lens** out)
{
    if (!ctx) return LVK_HIP_ERR_ARG;
    LVK_HIP_REQUIRE(ctx, out != nullptr);
    lvk_hip_lens* lens = new lvk_hip_lens;
    lens->ctx = ctx;
    const int rc = lvk_hip_lens_configure(lens, profile, test_mode);
    if (rc != LVK_HIP_OK) { delete lens; return rc; }
    *out = lens;
    return LVK_HIP_OK;
}

void lvk_hip_lens_destroy(lvk_hip_lens* lens)
{
    if (!lens) return;
    {
        lvk_device_guard guard(lens->ctx);
        lens->release_map();
    }
    delete lens;
}

// The view region of cv::getOptimalNewCameraMatrix for a rows x cols frame (x, y, w, h); the whole frame with no profile selected
int lvk_hip_lens_view(lvk_hip_lens* lens, int rows, int cols, int view_xywh[4])
{
    if (!lens) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = lens->ctx;
    LVK_HIP_REQUIRE(ctx, view_xywh != nullptr && rows > 0 && cols > 0);
    if (!lens->selected) { view_xywh[0] = view_xywh[1] = 0; view_xywh[2] = cols; view_xywh[3] = rows; return LVK_HIP_OK; }
    LensModel m;
    if (lvk_lens_model_build(lens->profile, rows, cols, m) != LVK_HIP_OK) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_lens_view: a frame of one row or column has no map");
    for (int i = 0; i < 4; i++) view_xywh[i] = m.view[i];
    return LVK_HIP_OK;
}

int lvk_hip_lens_apply(lvk_hip_lens* lens, void* d_src, int src_step, int rows, int cols, int format, void* d_dst, int dst_step)
{
    if (!lens) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = lens->ctx;
    LVK_HIP_ENTRY(ctx);
    LVK_HIP_REQUIRE(ctx, format == LVK_FORMAT_BGR || format == LVK_FORMAT_RGB || format == LVK_FORMAT_YUV);
    int rc = packed_pair_ok(lens, d_src, src_step, rows, cols, d_dst, dst_step, 3);
    if (rc != LVK_HIP_OK) return rc;
    const int yuv = format == LVK_FORMAT_YUV ? 1 : 0;
    if (lens->selected && (rc = lens->prepare(rows, cols)) != LVK_HIP_OK) return rc;
    // LCFilter.cpp:179-183: the grid goes into the frame the filter was handed, ahead of the warp
    if (lens->test_mode && (rc = lvk_launch_draw_grid(ctx, ctx->stream, d_src, src_step, rows, cols, kGridW, kGridH, yuv ? kMagentaYUV : kMagentaBGR, 1)) != LVK_HIP_OK) return rc;
    if (!lens->selected) return copy_frame(ctx, d_src, src_step, rows, cols, d_dst, dst_step, 3);
    return lvk_launch_remap_map(ctx, d_src, src_step, rows, cols, d_dst, dst_step, lens->d_map, lens->map_step(), kBackground, yuv, RemapLaunch{ctx->stream, ctx->remap_precision});
}

int lvk_hip_lens_apply_gray(lvk_hip_lens* lens, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step)
{
    if (!lens) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = lens->ctx;
    LVK_HIP_ENTRY(ctx);
    if (lens->test_mode) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_lens_apply_gray: the test-mode grid draws three bytes per pixel");
    int rc = packed_pair_ok(lens, d_src, src_step, rows, cols, d_dst, dst_step, 1);
    if (rc != LVK_HIP_OK) return rc;
    if (!lens->selected) return copy_frame(ctx, d_src, src_step, rows, cols, d_dst, dst_step, 1);
    if ((rc = lens->prepare(rows, cols)) != LVK_HIP_OK) return rc;
    return lvk_launch_remap_map_gray(ctx, d_src, src_step, rows, cols, d_dst, dst_step, lens->d_map, lens->map_step(), kBackground[0], RemapLaunch{ctx->stream});
}

int lvk_hip_lens_apply_c4(lvk_hip_lens* lens, const void* d_src, int src_step, int rows, int cols, int format, void* d_dst, int dst_step)
{
    if (!lens) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = lens->ctx;
    LVK_HIP_ENTRY(ctx);
    if (lens->test_mode) return ctx->fail(LVK_HIP_ERR_ARG, "lvk_hip_lens_apply_c4: the test-mode grid draws three bytes per pixel");
    LVK_HIP_REQUIRE(ctx, format == LVK_FORMAT_BGRA || format == LVK_FORMAT_RGBA);
    int rc = packed_pair_ok(lens, d_src, src_step, rows, cols, d_dst, dst_step, 4);
    if (rc != LVK_HIP_OK) return rc;
    // dword pixels, as the four-channel remaps take them -- with or without a profile
    LVK_HIP_REQUIRE(ctx, aligned_to(d_src, src_step, 4) && aligned_to(d_dst, dst_step, 4));
    if (!lens->selected) return copy_frame(ctx, d_src, src_step, rows, cols, d_dst, dst_step, 4);
    if ((rc = lens->prepare(rows, cols)) != LVK_HIP_OK) return rc;
    return lvk_launch_remap_map_c4(ctx, d_src, src_step, rows, cols, d_dst, dst_step, lens->d_map, lens->map_step(), kBackground, RemapLaunch{ctx->stream});
}

int lvk_hip_lens_apply_yuv420(lvk_hip_lens* lens, const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step,
                              void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int rows, int cols, int nv12)
{
    if (!lens) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = lens->ctx;
    LVK_HIP_ENTRY(ctx);
    const char* name = "lvk_hip_lens_apply_yuv420";
    LVK_HIP_REQUIRE(ctx, remap_precision_known(ctx->remap_precision));
    const PlaneSet src = plane_set(d_y, y_step, d_u, u_step, d_v, v_step, nv12, rows, cols), dst = plane_set(o_y, oy_step, o_u, ou_step, o_v, ov_step, nv12, rows, cols);
    LVK_HIP_REQUIRE(ctx, well_formed(src) && well_formed(dst, true));
    const Spans src_spans = spans_of(src);
    int rc = require_out_of_place(ctx, name, src_spans.s, src_spans.n, dst);
    if (rc != LVK_HIP_OK) return rc;
    if (lens->selected && (rc = lens->prepare(rows, cols)) != LVK_HIP_OK) return rc;

    // The packed source frame comes from the context's pool and goes back to it once the last kernel is enqueued: whoever is handed it next enqueues
    // behind that kernel on this context's stream (lvk_hip.h, lvk_hip_free), and the steady state allocates nothing.
    const int p_step = (3 * cols + 3) & ~3;
    void* d_packed = nullptr;
    if ((rc = lvk_hip_malloc(ctx, (size_t)p_step * rows, &d_packed)) != LVK_HIP_OK) return rc;
    rc = lvk_launch_ingest_yuv420(ctx, ctx->stream, d_y, y_step, d_u, u_step, d_v, v_step, nv12, rows, cols, d_packed, p_step);
    if (rc == LVK_HIP_OK && lens->test_mode) rc = lvk_launch_draw_grid(ctx, ctx->stream, d_packed, p_step, rows, cols, kGridW, kGridH, kMagentaYUV, 1);
    if (rc == LVK_HIP_OK)
        rc = lens->selected ? launch_remap_map_420(ctx, d_packed, p_step, dst, lens->d_map, lens->map_step(), kBackground)
                            : lvk_launch_egress_yuv420(ctx, ctx->stream, d_packed, p_step, rows, cols, o_y, oy_step, o_u, ou_step, o_v, ov_step, nv12);
    (void)lvk_hip_free(ctx, d_packed);
    return rc;
}

} // extern "C"
