/*
 * lvk_hip.h -- C-ABI of the MI355X-native LiveVisionKit stabilization hot path (liblvk_hip.so).
 *
 * This is the drop-in boundary: plain C, opaque handles, plain pointers and sizes, `int` status
 * (0 = ok, negative = error; lvk_hip_last_error() gives the text).  Nothing here throws and there are
 * no torch / OpenCV types.  Each entry point names the reference interface it replaces
 * (paths relative to the LiveVisionKit source tree).  The C++ facade in include/lvk/ (the
 * lvk::StabilizationFilter / lvk::VideoFilter API the OBS plugin compiles against) is a header-level
 * wrapper over these calls; INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - "d_" pointers are device (HBM) pointers valid on the context's device; all others are host pointers.
 *   - Frames are packed 8UC3 (the reference's cv::UMat CV_8UC3 layout, Data/VideoFrame.hpp:25) with a
 *     row pitch `step` in bytes, or planar 8UC1 where stated.
 *   - All work is enqueued on the context's HIP stream and is asynchronous, exactly like the
 *     reference's `run_(..., false)` kernel launches (Functions/Image.cpp:76); results are complete
 *     after lvk_hip_sync() (reference: Stopwatch::sync_gpu -> cv::ocl::finish, Timing/Stopwatch.cpp:127-131).
 *   - One context is driven by one host thread at a time; different contexts are independent
 *     (reference threading contract: SURVEY.md section 8b).  Every entry point makes its context's device current for
 *     the duration of the call and restores the caller's: a context of device 3 may be driven from a thread that never
 *     called hipSetDevice (one host thread + one context per GPU).
 *
 * Layout of this header
 *   PART 1 -- STABLE ABI: what a host of the reference binds (the filter, its frames and memory, the lvk:: image operations).
 *             A change that breaks one of these signatures or contracts increments LVK_HIP_ABI_VERSION.
 *   PART 2 -- EXPERIMENTAL / DIAGNOSTICS: per-stage entry points the parity tests drive, taps, profiling, the device-frame
 *             look-ahead.  They may change between builds of the library without a version increment; production hosts
 *             do not need them.
 */
#ifndef LVK_HIP_H
#define LVK_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LVK_HIP_OK              0
#define LVK_HIP_ERR_ARG        -1   /* violated pre-condition (the reference would LVK_ASSERT) */
#define LVK_HIP_ERR_RUNTIME    -2   /* HIP runtime error */
#define LVK_HIP_ERR_NO_DEVICE  -3   /* no usable gfx950 device / extension cannot run */

typedef struct lvk_hip_ctx lvk_hip_ctx;

/* =====================================================================================================================================
 * PART 1 -- STABLE ABI
 * ===================================================================================================================================== */

/* ---- context ------------------------------------------------------------------------------------
 * Replaces the implicit OpenCL context/queue of cv::ocl (Functions/OpenCL/Kernels.cpp:27-45).
 * lvk_hip_ctx_create makes its own non-blocking stream; lvk_hip_ctx_create_on_stream enqueues on the caller's
 * hipStream_t (NULL = the device's default stream) so the work is ordered with the caller's own GPU work. */
int  lvk_hip_ctx_create(int device, lvk_hip_ctx** out);
int  lvk_hip_ctx_create_on_stream(int device, void* hip_stream, lvk_hip_ctx** out);
void lvk_hip_ctx_destroy(lvk_hip_ctx* ctx);
int  lvk_hip_sync(lvk_hip_ctx* ctx);                 /* Stopwatch::sync_gpu, Timing/Stopwatch.cpp:127-131 */
void* lvk_hip_stream(lvk_hip_ctx* ctx);              /* the hipStream_t work is enqueued on */
const char* lvk_hip_last_error(lvk_hip_ctx* ctx);    /* NULL ctx: last error of a failed ctx_create */
const char* lvk_hip_version(void);                   /* human-readable build string */
/* ABI number of PART 1 of this header as the library was built (compare with LVK_HIP_ABI_VERSION of the header a host was compiled against;
 * tests/test_abi.py holds the two together). */
#define LVK_HIP_ABI_VERSION 12
int  lvk_hip_abi_version(void);
/* Devices of this process: contexts are addressed by HIP device index, and lvk_hip_device_count() is the number of indices worth trying -- the
 * highest gfx950 index + 1 (0 when there is no gfx950 device; never an error).  On the usual host every index below it is an MI355X; on a mixed
 * host (an integrated GPU or another architecture in between) lvk_hip_device_usable(d) says which indices lvk_hip_ctx_create accepts (the others
 * are refused with LVK_HIP_ERR_NO_DEVICE) -- or set HIP_VISIBLE_DEVICES.  One lvk_hip_ctx + one host thread per usable device is the multi-GPU
 * partitioning (no collective, no peer access). */
int  lvk_hip_device_count(void);
int  lvk_hip_device_usable(int device);

/* Ordering between contexts: everything enqueued so far on `producer` (its stream and the streams of its stabilizers) happens
 * before whatever is enqueued on `ctx` from now on.  GPU-side (an event per stream), no host wait.  What the reference gets from
 * OpenCV's single in-order OpenCL queue; needed here when a frame written on one context's stream is consumed on another's. */
int  lvk_hip_ctx_wait(lvk_hip_ctx* ctx, lvk_hip_ctx* producer);

/* ---- device memory helpers (for hosts without their own allocator) ------------------------------
 * Replace cv::UMat(USAGE_ALLOCATE_DEVICE_MEMORY) allocation / upload / download (Data/VideoFrame.cpp:27-29).
 * Like OpenCV's OpenCL buffer pool, lvk_hip_free keeps the block for the next lvk_hip_malloc of the same size (no device
 * synchronisation, no allocation in steady state; at most 4 GiB are kept, lvk_hip_trim gives them back).  A freed block may be
 * handed out again at once: work that still uses it must be on this context's stream, or have been fenced with lvk_hip_ctx_wait.
 * A block freed through another live context of the process goes back to the pool of the context that allocated it; freeing a block
 * that already sits in a pool (a double free) returns LVK_HIP_ERR_ARG. */
int lvk_hip_malloc(lvk_hip_ctx* ctx, size_t bytes, void** d_ptr);
int lvk_hip_free(lvk_hip_ctx* ctx, void* d_ptr);
int lvk_hip_trim(lvk_hip_ctx* ctx);
int lvk_hip_upload(lvk_hip_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);     /* async on the stream */
int lvk_hip_download(lvk_hip_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);   /* async on the stream */

/* pinned host memory for the planes of lvk_hip_stab_push_yuv420_host */
int  lvk_hip_host_malloc(lvk_hip_ctx* ctx, size_t bytes, void** h_ptr);      /* pinned, device-visible host memory */
int  lvk_hip_host_free(lvk_hip_ctx* ctx, void* h_ptr);


/* ---- a15/a16: dense remap ------------------------------------------------------------------------
 * lvk::remap(src, dst, homography, background, inverted=true)  (Functions/Image.cpp:85-151) running
 * easu_remap_homography (Functions/OpenCL/Sources/FSR.cl:407-452).  H = dst->src 3x3, row major, already
 * cast to float as Image.cpp:137-139 does.  (off_x, off_y) = ROI offset of dst (Image.cpp:121-123).
 * yuv != 0 <=> src.format == VideoFrame::YUV (selects the "-D YUV_INPUT" program, Image.cpp:36-41). */
int lvk_hip_remap_homography(lvk_hip_ctx* ctx,
                             const void* d_src, int src_step, int src_rows, int src_cols,
                             void* d_dst, int dst_step, int dst_rows, int dst_cols,
                             int off_x, int off_y, const float H[9], const uint8_t bg[3], int yuv);

/* lvk::remap(src, dst, offset_map, background) (Functions/Image.cpp:28-81, easu_remap FSR.cl:362-403) with the
 * offset map of WarpMesh::apply (Math/WarpMesh.cpp:190-191) evaluated inside the kernel from the mesh
 * vertices instead of being materialised (saves 4 full-resolution float2 passes).  `mesh` is a HOST pointer
 * to mesh_rows x mesh_cols x 2 floats of normalised backward offsets; dst has the size of src. */
int lvk_hip_remap_mesh(lvk_hip_ctx* ctx,
                       const void* d_src, int src_step, int src_rows, int src_cols,
                       void* d_dst, int dst_step,
                       const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3], int yuv);

/* lvk::remap(src, dst, offset_map, background) with a materialised map (Functions/Image.cpp:28-81, FSR.cl:362-403):
 * d_map = rows x cols float2 offsets in pixels resident in HBM (pitch map_step bytes); dst has the size of src. */
int lvk_hip_remap_map(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                      const void* d_map, int map_step, const uint8_t bg[3], int yuv);

/* Remap precision (opt-in; added to PART 1 without a version increment: no existing signature or contract changes, and EXACT is the default everywhere).
 * LVK_REMAP_1LSB runs the same EASU -- same 12 taps, same direction analysis, same normalised colours, same clamp and truncation -- with the twelve tap
 * weights algebraically regrouped: fewer instructions in the kernel that bounds a 4K stream, every output byte within 1 of EXACT's (the tolerance
 * SURVEY.md section 8c grants the remap; specification tests/np_easu_1lsb.py).  Border-band and background pixels never
 * reach the weights and are identical.
 * lvk_hip_set_remap_precision governs the stateless three-channel remap entries of THIS context: lvk_hip_remap_homography / _mesh / _map,
 * lvk_hip_warpmesh_apply, lvk_hip_warpmesh_apply_lens and lvk_hip_warpmesh_apply_yuv420.  A stabilizer has its own setting
 * (lvk_hip_stab_set_remap_precision) and is created EXACT whatever its context says.  Exact in every mode: the one- and four-channel remaps of PART 2,
 * lvk_hip_upscale and lvk_hip_sharpen with their `_gray` / `_c4` forms, lvk_hip_fsr_easu.  An unknown value is refused with LVK_HIP_ERR_ARG and changes nothing; get returns the
 * current value (LVK_HIP_ERR_ARG for a NULL context). */
#define LVK_REMAP_EXACT 0   /* bit-identical to the reference's kernels compiled for this chip (default) */
#define LVK_REMAP_1LSB  1   /* every output byte within 1 of EXACT; fewer instructions */
int lvk_hip_set_remap_precision(lvk_hip_ctx* ctx, int precision);
int lvk_hip_get_remap_precision(lvk_hip_ctx* ctx);

/* lvk::upscale(src, dst, size, yuv) (Functions/Image.cpp:155-202, kernel easu_scale FSR.cl:324-358): EASU upsampling of an
 * 8UC3 frame to dst_cols x dst_rows >= the source size (equal size = copy).  d_dst must not alias d_src. */
int lvk_hip_upscale(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                    void* d_dst, int dst_step, int dst_rows, int dst_cols, int yuv);

/* lvk::sharpen(src, dst, sharpness) (Functions/Image.cpp:206-233, kernel rcas FSR.cl:460-535): RCAS with sharpness in [0, 1].
 * OUT OF PLACE: the reference's ScalingFilter sharpens in place (Filters/ScalingFilter.cpp:57), where neighbour reads race
 * with writes; the defined result is that of distinct buffers, and aliasing is rejected.  Border pixels are copied. */
int lvk_hip_sharpen(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step, float sharpness);

/* Lens correction: the offset map LCFilter::prepare_undistort_maps builds
 * (Modules/OBS-Plugin/Sources/Enhancement/LCFilter.cpp:133-171) for a camera profile in the plugin's format
 * (Modules/OBS-Plugin/Sources/Tools/CCTool.cpp:120-153); LCFilter::filter == lvk_hip_remap_map with it. */
typedef struct lvk_camera_params { double fx, fy, cx, cy, k1, k2, p1, p2, k3; } lvk_camera_params;
int lvk_hip_lens_map_create(lvk_hip_ctx* ctx, const lvk_camera_params* params, int rows, int cols, void** d_map, int view_xywh[4]);
int lvk_hip_lens_map_destroy(lvk_hip_ctx* ctx, void* d_map);
/* FUSED lens mode (BASELINE config 5; this library's design, the reference only has the two-pass chain): the same warp in
 * closed form, composed into the coordinate of the stabilizing remap -> one EASU resampling, no map traffic.
 * lvk_hip_warpmesh_apply_lens == WarpMesh::apply applied to the lens-corrected frame, sampled from the RAW frame d_src;
 * lvk_hip_lens_undistort_points = raw tracking-frame points (scale sx, sy = frame / tracking size) -> corrected positions. */
int lvk_hip_warpmesh_apply_lens(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3], int yuv, const lvk_camera_params* lens);
int lvk_hip_lens_undistort_points(lvk_hip_ctx* ctx, const lvk_camera_params* params, int rows, int cols, double sx, double sy,
                                  const float* pts, int n, float* out);

/* WarpMesh::apply followed by the plugin's 4:2:0 egress (I4XXIngest / NV12Ingest::to_obs, Modules/OBS-Plugin/Interop/FrameIngest.cpp:
 * 540-557,590-602) in one kernel: packed YUV 8UC3 in, I420 (y, u, v) or NV12 (y, uv; o_v ignored) planes out, even dimensions.
 * Bit-identical to lvk_hip_warpmesh_apply + lvk_hip_egress_yuv420. */
int lvk_hip_warpmesh_apply_yuv420(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                                  void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int nv12,
                                  const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3]);

/* WarpMesh::apply(src, dst, background) (Math/WarpMesh.cpp:183-223): a 2x2 mesh goes through
 * cv::getPerspectiveTransform + the homography kernel, anything larger through the mesh kernel. */
int lvk_hip_warpmesh_apply(lvk_hip_ctx* ctx,
                           const void* d_src, int src_step, int rows, int cols,
                           void* d_dst, int dst_step,
                           const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[3], int yuv);

/* ---- section 8f row 2: YUV420 <-> packed YUV444 either side of the filter --------------------------------------
 * I4XXIngest::to_ocl / NV12Ingest::to_ocl (Modules/OBS-Plugin/Interop/FrameIngest.cpp:494-522,567-585): chroma
 * cv::resize(INTER_LINEAR) + merge into the packed 8UC3 frame the filter consumes; and ::to_obs (:526-557,589-602):
 * split + cv::resize(0.5, 0.5, INTER_AREA).  nv12 != 0: d_u is the interleaved UV plane and d_v is ignored.
 * rows and cols must be even. */
int lvk_hip_ingest_yuv420(lvk_hip_ctx* ctx, const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step, int nv12,
                          int rows, int cols, void* d_dst, int dst_step);
int lvk_hip_egress_yuv420(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                          void* d_y, int y_step, void* d_u, int u_step, void* d_v, int v_step, int nv12);

/* Every video format FrameIngest::Select accepts (Modules/OBS-Plugin/Interop/FrameIngest.cpp:36-75): video_format is libobs' enum video_format
 * (media-io/video-io.h of libobs 27.2.4), i.e. obs_source_frame::format passed through.  d_planes / steps = the frame's data[] / linesize[] on the
 * device (3 entries; unused ones NULL / 0; the alpha planes of I40A / I42A / YUVA are not touched, as in the reference).
 *   I420 / I40A / NV12            -> lvk_hip_ingest_yuv420 / lvk_hip_egress_yuv420 above (I4XXIngest, NV12Ingest)
 *   I422 / I42A                   I4XXIngest with chroma (cols / 2) x rows: INTER_LINEAR upsampling of the width in, INTER_AREA (0.5, 1.0) out (:494-557)
 *   I444 / YUVA                   merge / split (:521,531)
 *   YUY2 / YVYU / UYVY            P422Ingest::to_ocl / to_obs (:615-666): 2 bytes per pixel, chroma shared by a pixel pair
 *   AYUV                          P444Ingest (:679-703): the last three of A Y U V in; A = 255 out
 *   Y800 / BGR3                   DirectIngest (:728-753): the bytes as they are (Y800: a one-channel frame, which lvk_hip_stab_push and the plane entries
 *                                 refuse like the reference's lvk::remap does, Functions/Image.cpp:32; lvk_hip_stab_push_gray of PART 2 takes it)
 *   RGBA / BGRA / BGRX            DirectIngest as written: rows * cols * 3 BYTES from data[0] viewed as 3-byte pixels (:743-747) -- the colour planes are
 *                                 not separated; steps[0] must be 4 * cols.  Reproduced, not endorsed.
 * cols even for the 4:2:2 formats, rows and cols even for 4:2:0.  The frame is 8UC3 (Y800: 8UC1) of rows x cols; lvk_hip_obs_frame_format gives the
 * LVK_FORMAT_* its pixels carry (the VideoFrame::Format each ingest declares), negative for a format FrameIngest::Select rejects. */
#define LVK_VIDEO_FORMAT_I420 1
#define LVK_VIDEO_FORMAT_NV12 2
#define LVK_VIDEO_FORMAT_YVYU 3
#define LVK_VIDEO_FORMAT_YUY2 4
#define LVK_VIDEO_FORMAT_UYVY 5
#define LVK_VIDEO_FORMAT_RGBA 6
#define LVK_VIDEO_FORMAT_BGRA 7
#define LVK_VIDEO_FORMAT_BGRX 8
#define LVK_VIDEO_FORMAT_Y800 9
#define LVK_VIDEO_FORMAT_I444 10
#define LVK_VIDEO_FORMAT_BGR3 11
#define LVK_VIDEO_FORMAT_I422 12
#define LVK_VIDEO_FORMAT_I40A 13
#define LVK_VIDEO_FORMAT_I42A 14
#define LVK_VIDEO_FORMAT_YUVA 15
#define LVK_VIDEO_FORMAT_AYUV 16
int lvk_hip_ingest_obs(lvk_hip_ctx* ctx, int video_format, const void* const d_planes[3], const int steps[3], int rows, int cols, void* d_dst, int dst_step);
int lvk_hip_egress_obs(lvk_hip_ctx* ctx, int video_format, const void* d_src, int src_step, int rows, int cols, void* const d_planes[3], const int steps[3]);
int lvk_hip_obs_frame_format(int video_format);

/* ---- a1/a2: the stabilization filter ----------------------------------------------------------------------
 * lvk_stab_settings flattens lvk::StabilizationFilterSettings (Filters/StabilizationFilter.hpp:28-39) and its bases
 * FrameTrackerSettings (Vision/FrameTracker.hpp:31-44) : FeatureDetectorSettings (Vision/FeatureDetector.hpp:28-37) and
 * PathSmootherSettings (Vision/PathSmoother.hpp:29-39); same names, same defaults (lvk_stab_default_settings). */
typedef struct lvk_stab_settings
{
    int detection_width, detection_height;          /* detection_resolution {256, 256} */
    int detection_regions_x, detection_regions_y;   /* detection_regions {2, 2} */
    int force_detection;                            /* false */
    float max_feature_density, min_feature_density, accumulation_rate;    /* 0.20, 0.05, 2.0 */
    int track_local_motions;                        /* true */
    float temporal_smoothing, local_smoothing;      /* 1.0, 20.0 */
    int min_motion_samples;                         /* 75 */
    float acceptance_threshold, uniformity_threshold;                     /* 8.0, 0.20 */
    int predictive_samples;                         /* 10 */
    float corrective_limit_x, corrective_limit_y;   /* corrective_limits {0.1, 0.1} */
    float smoothing_steps, response_rate;           /* 20.0, 0.04 */
    int motion_width, motion_height;                /* StabilizationFilterSettings::motion_resolution {2, 2} */
    float background[3];                            /* background_colour {255, 0, 255} */
    int crop_to_stable_region, stabilize_output;    /* false, true */
    float min_scene_quality, min_tracking_quality;  /* 0.8, 0.3 */
} lvk_stab_settings;

typedef struct lvk_stab_stats
{
    float tracking_stability;      /* FrameTracker::tracking_stability() */
    float scene_quality, trust;    /* m_SceneQuality, m_TrustFactor */
    float distribution;            /* FeatureDetector::detect() return value of the last frame */
    int n_detected, n_matched, n_tracked, frame_delay;
    double smoothing_factor;       /* PathSmoother m_SmoothingFactor */
    double homography[9];          /* last global motion estimate (tracking-resolution pixels) */
} lvk_stab_stats;

/* lvk::VideoFrame::Format (Data/VideoFrame.hpp:27) */
#define LVK_FORMAT_BGR 0
#define LVK_FORMAT_BGRA 1
#define LVK_FORMAT_RGB 2
#define LVK_FORMAT_RGBA 3
#define LVK_FORMAT_YUV 4
#define LVK_FORMAT_GRAY 5

typedef struct lvk_hip_stab lvk_hip_stab;

void lvk_stab_default_settings(lvk_stab_settings* s);
/* StabilizationFilter(settings) / configure(settings) (Filters/StabilizationFilter.cpp:34-65) */
int  lvk_hip_stab_create(lvk_hip_ctx* ctx, const lvk_stab_settings* settings, lvk_hip_stab** out);
void lvk_hip_stab_destroy(lvk_hip_stab* stab);
int  lvk_hip_stab_configure(lvk_hip_stab* stab, const lvk_stab_settings* settings);
int  lvk_hip_stab_restart(lvk_hip_stab* stab);            /* :139-144 */
/* Debug overlays into the newest queued frame, i.e. the caller's borrowed buffer of the last push (StabilizationFilter.cpp:163-188;
 * kernels Functions/OpenCL/Sources/Drawing.cl:22-39,75-105): crosses at the tracked features coloured lerp(RED, GREEN, trust);
 * BLUE grid with motion_resolution - 1 cells.  Asynchronous on the context's stream. */
int  lvk_hip_stab_draw_trackers(lvk_hip_stab* stab);
int  lvk_hip_stab_draw_motion_mesh(lvk_hip_stab* stab);
/* lvk::draw_grid / lvk::draw_crosses on a packed 8UC3 device frame (Functions/Drawing.tpp:53-93,146-196); pts_xy = n host (x, y)
 * floats, scaled by (scale_x, scale_y) and rounded to pixels like cv::multiply(.., CV_32S). */
int  lvk_hip_draw_grid(lvk_hip_ctx* ctx, void* d_dst, int dst_step, int rows, int cols, int grid_w, int grid_h, const uint8_t colour[3], int thickness);
int  lvk_hip_draw_crosses(lvk_hip_ctx* ctx, void* d_dst, int dst_step, int rows, int cols, const float* pts_xy, int n,
                          float scale_x, float scale_y, const uint8_t colour[3], int cross_size, int thickness);
/* The test-mode HUD, drawn on the device (the reference maps the frame to the host for cv::rectangle / cv::putText): lvk::draw_points,
 * lvk::draw_rect and lvk::draw_text (Functions/Drawing.tpp:40-49,95-141,198-218; VSFilter::draw_debug_hud, VSFilter.cpp:368-383), IN PLACE
 * on a packed 8UC3 device frame of any pitch and byte alignment; only bytes inside cols * 3 of a row are written.  Asynchronous on the
 * context's stream.  Whatever lies outside the frame is clipped; a call that draws nothing (n == 0, an empty string, a shape wholly outside
 * the frame) is a valid no-op.  A refused call (LVK_HIP_ERR_ARG) leaves the frame untouched.  Specification: tests/np_draw.py.
 *   points  the `points` kernel (Drawing.cl:43-69): pts_xy as for lvk_hip_draw_crosses; each point is the square of half width
 *           (point_size + 1) / 2, x in [max(px - h, 0), min(px + h, cols)), y alike.  Refused: point_size < 1, a negative scale.
 *   rect    rect_xywh = (x, y, w, h), corners (x0, y0) = (x, y), (x1, y1) = (x + w - 1, y + h - 1).  thickness t >= 1: with a = t / 2 and
 *           b = (t - 1) / 2 the pixels of [x0 - a, x1 + b] x [y0 - a, y1 + b] that are not strictly inside (x0 + b, x1 - a) x (y0 + b, y1 - a);
 *           t = 1 is the outline cv::rectangle(Rect) draws, above that the band has SQUARE corners where OpenCV rounds the joins of its
 *           thick lines.  t < 0 fills the rectangle (cv::FILLED).  Refused: t == 0, w <= 0 or h <= 0, a call of 2^31 pixels or more.
 *   text    the library's OWN fixed-cell font, not OpenCV's Hershey glyphs: 5 x 7 glyphs in a 6 x 9 cell for the bytes 0x20 .. 0x7E, any other
 *           byte draws as '?'.  (x, y) is the bottom-left corner of the baseline as for cv::putText: font pixel (c, r) of character i is the
 *           scale x scale block at (x + (6 i + c) scale, y - (7 - r) scale), grown by (thickness - 1) / 2 pixels on each side.  One launch a
 *           string.  Refused: a string of more than 256 bytes, scale outside [1, 32767], thickness outside [1, 65535]. */
int  lvk_hip_draw_points(lvk_hip_ctx* ctx, void* d_dst, int dst_step, int rows, int cols, const float* pts_xy, int n, float scale_x, float scale_y,
                         const uint8_t colour[3], int point_size);
int  lvk_hip_draw_rect(lvk_hip_ctx* ctx, void* d_dst, int dst_step, int rows, int cols, const int rect_xywh[4], const uint8_t colour[3], int thickness);
int  lvk_hip_draw_text(lvk_hip_ctx* ctx, void* d_dst, int dst_step, int rows, int cols, const char* text, int x, int y, const uint8_t colour[3],
                       int scale, int thickness);
/* Fused lens pre-warp for the stream this filter stabilizes: frames are pushed RAW (uncorrected); the tracker estimates the
 * motion between lens-corrected feature positions and the output remap composes lens map and stabilizing warp.
 * params = NULL switches it off.  Restarts the filter (queued frames are dropped). */
int  lvk_hip_stab_set_lens(lvk_hip_stab* stab, const lvk_camera_params* params);
int  lvk_hip_stab_reset_context(lvk_hip_stab* stab);      /* :155-159 */
int  lvk_hip_stab_ready(const lvk_hip_stab* stab);        /* :148-151 */
int  lvk_hip_stab_frame_delay(const lvk_hip_stab* stab);  /* :192-195 */
int  lvk_hip_stab_stable_region(const lvk_hip_stab* stab, int rows, int cols, int rect_xywh[4]);   /* :199-205 */

/* VideoFilter::apply(std::move(input), output) -> StabilizationFilter::filter (Filters/VideoFilter.cpp:46-51,
 * Filters/StabilizationFilter.cpp:69-135).  d_frame: packed 8UC3 device frame; like the reference's moved-in
 * input it is BORROWED (not copied) until it has been emitted `frame_delay` pushes later -- `*released` then
 * returns its pointer (or NULL); the caller may reuse that buffer once the stream has passed this call.
 * d_out receives the stabilized delayed frame when *produced == 1 (and carries *out_timestamp = that frame's
 * timestamp, Math/WarpMesh.cpp:221-222); *produced == 0 while the delay builds ("output.release()").
 * The output remap is only enqueued: call lvk_hip_sync() before reading d_out on the host.
 *
 * SIZE OF THE OUTPUT.  The queue holds whole frames (StabilizationFilter.cpp:118-131) and the emitted frame is the DELAYED one, at ITS
 * OWN size and format (WarpMesh::apply allocates dst from the delayed source, Math/WarpMesh.cpp:183-223 -> Functions/Image.cpp:53,116):
 * when the frame size changes in the middle of a stream (an OBS source that is resized -- VSFilter.cpp:352-364 does not restart its
 * filter), the next `frame_delay` pushes still emit frames of the OLD size.  lvk_hip_stab_next_output() tells the caller, before the
 * push, whether the push of a rows x cols frame will emit and what (1 / 0; *out = the delayed frame's rows, cols, format) -- size d_out
 * from it.  d_out is a buffer of out_rows rows of out_step bytes: a push whose output would not fit (out_step < 3 * cols or out_rows <
 * rows of the frame to be emitted, or d_out == NULL when a frame is due) is REFUSED with LVK_HIP_ERR_ARG BEFORE anything changes -- the
 * frame is not queued, nothing is released, the filter is as it was; the same push with a large enough d_out then succeeds.  The rows x
 * cols top-left part of d_out is written, nothing else.  *emitted (optional) = geometry and format of the frame written to d_out. */
typedef struct lvk_frame_info { int rows, cols, format; } lvk_frame_info;
int  lvk_hip_stab_next_output(const lvk_hip_stab* stab, int rows, int cols, int format, lvk_frame_info* out);
int  lvk_hip_stab_push(lvk_hip_stab* stab, const void* d_frame, int step, int rows, int cols, uint64_t timestamp, int format,
                       void* d_out, int out_step, int out_rows, int* produced, uint64_t* out_timestamp, const void** released,
                       lvk_frame_info* emitted);

/* The OBS asynchronous path in one call (Modules/OBS-Plugin/Interop/VisionFilter.cpp:151-212): YUV 4:2:0 planes in
 * (I420, or NV12 with nv12 != 0 and d_u = interleaved UV), ingest -> filter -> egress, 4:2:0 planes out.  The packed
 * frames the filter queues live in an internal pool; a warped frame leaves through one kernel that remaps and writes the planes.
 * Input planes are consumed when the call returns; output planes are complete after lvk_hip_sync().  A filter is fed EITHER
 * through this call OR through lvk_hip_stab_push -- switching needs lvk_hip_stab_restart() (the two own their queued frames
 * differently).
 * SIZE OF THE OUTPUT: as for lvk_hip_stab_push -- the emitted frame is the DELAYED one at its own size (the reference's queue holds whole
 * frames, StabilizationFilter.cpp:118-131), so after rows / cols CHANGE in the middle of a stream the next `frame_delay` pushes emit frames of
 * the OLD size (round 6; rounds 2-5 dropped them).  lvk_hip_stab_next_output(stab, rows, cols, LVK_FORMAT_YUV, &info) says what the push will
 * emit; the output planes hold o_rows luma rows (o_rows / 2 chroma rows) at the given pitches, and a push whose output would not fit is refused
 * with LVK_HIP_ERR_ARG before the filter changes.  *emitted (optional) = the geometry of the frame written. */
int  lvk_hip_stab_push_yuv420(lvk_hip_stab* stab, const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step, int nv12,
                              int rows, int cols, uint64_t timestamp,
                              void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int o_rows,
                              int* produced, uint64_t* out_timestamp, lvk_frame_info* emitted);
/* The same call for ANY three-channel video format FrameIngest::Select accepts; Y800, a one-channel frame, goes through lvk_hip_stab_push_gray of PART 2.
 * video_format is an LVK_VIDEO_FORMAT_*; d_planes / steps are as for lvk_hip_ingest_obs; o_planes / o_steps / o_rows are the planes of the emitted frame
 * and their row capacity.  I420 / I40A / NV12 take lvk_hip_stab_push_yuv420's route; the other formats
 * are converted into the filter's frame pool (FrameIngest::to_ocl), pushed, and the emitted frame -- the DELAYED one, at its own size -- converted back
 * (::to_obs).  Input planes consumed when the call returns; output planes complete after lvk_hip_sync(); planes that cannot hold the emitted frame are
 * refused before anything changes.  Shares the frame queue with lvk_hip_stab_push_yuv420.
 * FORMAT CLASS (declared deviation): the emitted frame leaves in the video format of the push that emits it, which converts it only within its format
 * class (the YUV formats, which all queue the same packed frame).  A push whose delayed frame is of the other class (BGR3 / BGRA / BGRX / RGBA frames
 * queued and a YUV push, or the reverse -- lvk_hip_stab_next_output reports the delayed frame's format) is refused with LVK_HIP_ERR_ARG before anything
 * changes, by this call and by lvk_hip_stab_push_yuv420 alike; lvk_hip_stab_restart() lets the new format through.  The reference converts the delayed
 * frame into its own OBS frame (OBSFrame::to_obs_frame, viewAsFormat); this call takes one format per push and does not convert between BGR / RGB and YUV.
 * Planes that FrameIngest::to_ocl could not read (a NULL plane, a short step, an odd width where the format subsamples, rows or cols <= 0) are likewise
 * refused before anything changes. */
int  lvk_hip_stab_push_obs(lvk_hip_stab* stab, int video_format, const void* const d_planes[3], const int steps[3], int rows, int cols, uint64_t timestamp,
                           void* const o_planes[3], const int o_steps[3], int o_rows, int* produced, uint64_t* out_timestamp, lvk_frame_info* emitted);

/* The same path for frames that live in HOST memory -- FrameIngest::upload_planes -> to_ocl -> filter -> to_obs -> download_planes
 * (Modules/OBS-Plugin/Interop/FrameIngest.cpp:415-474,494-602): h_* / oh_* are planes in PINNED host memory (lvk_hip_host_malloc,
 * hipHostMalloc or hipHostRegister; contiguous planes, the OBS layout, travel as one copy).  The library schedules the transfers: luma
 * first (the tracker starts while the chroma planes are still on the link), one upload stream; the output planes are written by the
 * remap kernel ITSELF, straight into the pinned host planes (zero copy; the download route -- remap to device planes, then a D2H copy --
 * is kept behind LVK_HIP_HOST_SINK=copy for comparison: the runtime performs that copy with a blit kernel that is slower for every
 * caller measured) -- same pixels.  Input planes are consumed when the call returns; output planes are complete after
 * lvk_hip_sync().  rows and cols even.  Shares the frame queue with lvk_hip_stab_push_yuv420 (the two may be mixed), and its output sizing: the
 * output planes have the DELAYED frame's size (lvk_hip_stab_next_output), o_rows luma rows of capacity.  Pageable plane
 * pointers are refused with LVK_HIP_ERR_ARG: both ends of every plane are looked up on every call (an address that was pinned once may
 * have been freed and handed out again as pageable memory). */
int  lvk_hip_stab_push_yuv420_host(lvk_hip_stab* stab, const void* h_y, int y_step, const void* h_u, int u_step, const void* h_v, int v_step, int nv12,
                                   int rows, int cols, uint64_t timestamp,
                                   void* oh_y, int oy_step, void* oh_u, int ou_step, void* oh_v, int ov_step, int o_rows,
                                   int* produced, uint64_t* out_timestamp, lvk_frame_info* emitted);
/* The host entry for ANY three-channel video format FrameIngest::Select accepts (ABI 12); Y800, a one-channel frame, goes through lvk_hip_stab_push_gray_host
 * of PART 2.  It is the contract of lvk_hip_stab_push_obs with h_planes / oh_planes
 * in PINNED host memory -- what FrameIngest::upload_planes / download_planes do for every format alike (FrameIngest.cpp:415-474).  I420 / I40A / NV12
 * are handed to lvk_hip_stab_push_yuv420_host unchanged (as lvk_hip_stab_push_obs hands them to lvk_hip_stab_push_yuv420).  Plane geometry per format
 * as for lvk_hip_ingest_obs / lvk_hip_egress_obs: 4:2:2 planar chroma cols / 2 wide and rows high; packed 4:2:2 2 * cols bytes a row; AYUV 4 * cols;
 * BGR3 3 * cols; RGBA / BGRA / BGRX rows * cols * 3 bytes of data[0] with steps[0] == 4 * cols, as the reference moves them; alpha planes are never
 * touched.  The library schedules the transfers: one upload stream into staging planes sized for the format, planes that are contiguous in host
 * memory as one copy, the luma plane of a planar format first (the tracker starts on it; packed formats travel whole); the output planes are written
 * by the kernels THEMSELVES straight into the pinned host planes (the fused remap + egress sinks; BGR3 / RGBA / BGRA / BGRX, which have no fused sink:
 * remap, then the egress into the host planes) -- there is no download route through device planes.  Input planes are consumed when the call returns;
 * output planes are complete after lvk_hip_sync().  Shares the frame queue with lvk_hip_stab_push_obs, lvk_hip_stab_push_yuv420 and
 * lvk_hip_stab_push_yuv420_host: the four may be mixed within a format class.  After a resize the next `frame_delay` outputs have the old size.
 * REFUSED with LVK_HIP_ERR_ARG before anything changes (nothing queued or uploaded; the same push with good arguments then succeeds): everything
 * lvk_hip_stab_push_obs refuses (a NULL plane, a short step, an odd width where the format subsamples, sizes <= 0, Y800 and unknown formats, output
 * planes that cannot hold the DELAYED frame at its own size -- lvk_hip_stab_next_output --, a delayed frame of the other format class); an input or
 * output plane that is pageable memory at either end of its extent; a push while frames announced through lvk_hip_stab_prefetch_yuv420_host are
 * outstanding.  LOOK-AHEAD is out of scope for these formats: lvk_hip_stab_prefetch_yuv420_host announces 4:2:0 frames only. */
int  lvk_hip_stab_push_obs_host(lvk_hip_stab* stab, int video_format,
                                const void* const h_planes[3], const int steps[3], int rows, int cols, uint64_t timestamp,
                                void* const oh_planes[3], const int o_steps[3], int o_rows,
                                int* produced, uint64_t* out_timestamp, lvk_frame_info* emitted);
/* Look-ahead for streaming callers (the reader thread of VideoFilter::stream, Filters/VideoFilter.cpp:62-209, uploads ahead of the
 * filter thread): starts the upload of the planes that the NEXT lvk_hip_stab_push_yuv420_host call will push (same pointers), so that
 * the link carries frame n + 1 while frame n is tracked: announce frame n + 1, then push frame n.  Announced frames are pushed in the
 * order announced, at most two outstanding; the planes stay the caller's until their push returns. */
int  lvk_hip_stab_prefetch_yuv420_host(lvk_hip_stab* stab, const void* h_y, int y_step, const void* h_u, int u_step, const void* h_v, int v_step,
                                       int nv12, int rows, int cols);
/* Forget the frames that were announced and not pushed (a caller that stops, seeks or switches buffers after announcing frame n + 1 --
 * VideoFilter::stream's reader thread ending on a failed read, Filters/VideoFilter.cpp:77-103).  Returns once their uploads no longer
 * read the caller's planes.  lvk_hip_stab_restart() implies it. */
int  lvk_hip_stab_prefetch_cancel(lvk_hip_stab* stab);
/* Optional: run the bulk kernels (4:2:0 ingest, the output remap) on a second, low-priority HIP stream so that they overlap the
 * tracking of the next frame (the reference gets the same effect from OpenCL's asynchronous `run_(..., false)` launches,
 * Functions/Image.cpp:76); the remap then uses its occupancy-capped variants.  With overlap enabled d_out is complete only after
 * lvk_hip_sync(), and *released reports a borrowed frame one push later (after its remap has finished).
 * Ordering: INPUTS need nothing from the caller -- whatever was enqueued on the context's stream before a push (the decode / copy that
 * fills the frame or the planes) is made visible to the bulk stream by an event the push records.  OUTPUTS are produced on the
 * bulk stream: consume them there (lvk_hip_stab_output_stream) or after lvk_hip_sync(); reusing the same output buffer for the
 * next push is safe (same stream).  Frames dropped outside a push (queue shrunk by configure, mode toggled) come back through
 * *released of the following pushes. */
int  lvk_hip_stab_set_overlap(lvk_hip_stab* stab, int enable);
/* The same mode on a stream the caller owns: the bulk kernels run on the stream of `bulk` (a second context on the same device; NULL
 * switches overlap off).  For hosts whose output frames outlive the stabilizer or feed stream-ordered consumers: outputs belong to `bulk`. */
int  lvk_hip_stab_set_bulk_context(lvk_hip_stab* stab, lvk_hip_ctx* bulk);
/* The hipStream_t the outputs of the following pushes are produced on (the bulk stream in overlap mode, else the context's
 * stream): enqueue stream-ordered consumers of d_out / the output planes (a D2H copy, an encoder) there instead of calling
 * lvk_hip_sync().  Changes when lvk_hip_stab_set_overlap or stabilize_output change. */
void* lvk_hip_stab_output_stream(lvk_hip_stab* stab);
/* The remap precision of THIS stabilizer's output (LVK_REMAP_EXACT / LVK_REMAP_1LSB, see lvk_hip_set_remap_precision): takes effect on the next emitted
 * frame -- the queue, the trajectory and the tracker's state are kept, nothing restarts, no stream is waited for.  Valid with overlap on or off and for
 * every push entry; the GRAY pushes of PART 2 accept the setting and stay exact.  A stabilizer is created EXACT.  An unknown value is refused with
 * LVK_HIP_ERR_ARG and changes nothing. */
int  lvk_hip_stab_set_remap_precision(lvk_hip_stab* stab, int precision);
int  lvk_hip_stab_get_remap_precision(const lvk_hip_stab* stab);


/* ---- the deblocking filter ----------------------------------------------------------------------------------------------------------
 * lvk::DeblockingFilter (Filters/DeblockingFilter.{hpp,cpp}; the OBS plugin's "ADB" filter and the editor's `adb` stage): blends a median-
 * smoothed copy of the frame into it where its macroblocks are flat.  lvk_deblock_settings = DeblockingFilterSettings (DeblockingFilter.hpp:
 * 27-33), same names and defaults (lvk_hip_deblock_default_settings: 3, 16, 5, 4.0f).  create / configure refuse (LVK_HIP_ERR_ARG, nothing
 * changes) a settings struct unless block_size > 0, filter_size >= 3 and odd, detection_levels > 0 and filter_scaling > 1 (:35-45). */
typedef struct lvk_deblock_settings
{
    uint32_t detection_levels;     /* 3 */
    uint32_t block_size;           /* 16 */
    uint32_t filter_size;          /* 5 */
    float filter_scaling;          /* 4.0f */
} lvk_deblock_settings;

typedef struct lvk_hip_deblock lvk_hip_deblock;

void lvk_hip_deblock_default_settings(lvk_deblock_settings* s);
int  lvk_hip_deblock_create(lvk_hip_ctx* ctx, const lvk_deblock_settings* settings, lvk_hip_deblock** out);   /* settings NULL: defaults */
int  lvk_hip_deblock_configure(lvk_hip_deblock* deb, const lvk_deblock_settings* settings);                    /* :35-45 */
void lvk_hip_deblock_destroy(lvk_hip_deblock* deb);
/* VideoFilter::apply(frame, frame) -> DeblockingFilter::filter (:48-110), IN PLACE on a packed 8UC3 device frame of any pitch (step >= 3 * cols)
 * of format LVK_FORMAT_BGR, _RGB or _YUV.  Only the region of whole block_size x block_size macroblocks at the top left is written; *region_xywh
 * (optional) = that region.  Refused with LVK_HIP_ERR_ARG before anything changes (frame and filter as they were): GRAY and 4-channel formats,
 * a frame without one whole macroblock or whose 1 / filter_scaling downscale is empty (the reference throws from cv::resize), filter_size > 255.
 * Asynchronous on the context's stream; the first call at a new geometry builds its interpolation tables.  GRAY and BGRA / RGBA frames go through
 * lvk_hip_deblock_apply_gray / _c4 of PART 2, on the same handle. */
int  lvk_hip_deblock_apply(lvk_hip_deblock* deb, void* d_frame, int step, int rows, int cols, int format, int region_xywh[4]);
/* DeblockingFilter::draw_influence (:114-131): blends MAGENTA[format] into the region of the last apply with that apply's blend maps.  Refused
 * before the first apply and when that region does not fit the frame. */
int  lvk_hip_deblock_draw_influence(const lvk_hip_deblock* deb, void* d_frame, int step, int rows, int cols, int format);
int  lvk_hip_deblock_filter_region(const lvk_hip_deblock* deb, int region_xywh[4]);       /* :135-138; (0, 0, 0, 0) before the first apply */

/* ---- contrast adaptive sharpening ---------------------------------------------------------------------------------------------------
 * The OBS plugin's CAS filter (Sources/Enhancement/CASFilter.cpp, Effects/CASEffect.cpp, the FidelityFX CasFilter of cas.effect with CAS_SLOW
 * and CAS_BETTER_DIAGONALS): d_dst = CAS(d_src), OUT OF PLACE, on a packed frame of format LVK_FORMAT_BGR, _RGB or _YUV (3 channels) or
 * LVK_FORMAT_BGRA, _RGBA (4 channels; the 4th byte is written as 255, the shader's float4(col, 1.0)).  Every channel is sharpened on its own,
 * the neighbours outside the frame read as 0, and only the cols * channels bytes of each destination row are written (any pitch, any byte
 * alignment).  sharpness in [0, 1] (the filter's default is 0.8).  Refused with LVK_HIP_ERR_ARG, the destination untouched: GRAY or
 * unknown formats, sharpness outside [0, 1] or NaN, rows or cols <= 0, a step < cols * channels, a NULL pointer, and source and destination
 * byte ranges that overlap (in place would race: CAS reads its neighbours).  Asynchronous on the context's stream. */
int  lvk_hip_cas(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, int format, void* d_dst, int dst_step, float sharpness);

/* ---- format conversion --------------------------------------------------------------------------------------------------------------
 * VideoFrame::reformatTo (Data/VideoFrame.cpp:170-301; OpenCV's CPU 8-bit cvtColor): d_dst = the d_src frame of format src_format
 * converted to dst_format, OUT OF PLACE, both packed (LVK_FORMAT_BGR, _RGB, _YUV: 3 channels; _BGRA, _RGBA: 4; _GRAY: 1).  Integer
 * arithmetic, bit-exact: grey is RGB2Gray<uchar> (15-bit), YUV is RGB2YCrCb_i / YCrCb2RGB_i<uchar> with the YUV coefficients (14-bit),
 * BGRA / RGBA -> YUV goes through the 3-channel frame, YUV -> GRAY is channel 0, GRAY -> YUV is (g, 128, 128), BGRA <-> RGBA keeps the alpha, and an added
 * alpha is 255 (YUV -> BGRA / RGBA included: the reference's own call leaves its destination stale, VideoFrame.cpp:262,264).  src_format == dst_format
 * is a 2-D copy.  Only the cols * channels bytes of each destination row are written (any pitch, any byte alignment).  Refused with
 * LVK_HIP_ERR_ARG, the destination untouched: an unknown format, rows or cols <= 0, a step < cols * channels, a NULL pointer, and source
 * and destination byte ranges that overlap.  Asynchronous on the context's stream. */
int  lvk_hip_reformat(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, int src_format, void* d_dst, int dst_step,
                      int dst_format);

/* ---- FSR scaling ------------------------------------------------------------------------------------------------------------------
 * The OBS plugin's FSR filter (Sources/Scaling/FSRFilter.cpp, Effects/FSREffect.cpp, the FidelityFX FSR 1 EASU pass of fsr.effect; no
 * RCAS: chain lvk_hip_cas): d_dst (out_rows x out_cols) = EASU of the region (x, y, w, h) of d_src, OUT OF PLACE, for any output size (up,
 * down, anisotropic).  Taps at the region's edge read the frame outside it; taps outside the frame read its edge (clamp-to-edge).  Packed
 * frames of format LVK_FORMAT_BGR, _RGB or _YUV (3 channels) or LVK_FORMAT_BGRA, _RGBA (4 channels; the 4th byte is written as 255); the
 * luma weighs red, green and blue (bytes 0, 1, 2 of YUV).  Only the out_cols * channels bytes of each destination row are written (any
 * pitch, any byte alignment).  Refused with LVK_HIP_ERR_ARG, the destination untouched: GRAY or unknown formats, rows, cols, out_rows or
 * out_cols <= 0, a region that is empty or not inside the frame, a step smaller than its row, a NULL pointer, and source and destination
 * byte ranges that overlap.  Asynchronous on the context's stream. */
int  lvk_hip_fsr_easu(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, int format, const int region_xywh[4], void* d_dst,
                      int dst_step, int out_rows, int out_cols);
/* FSRFilter::tick + FSREffect::should_skip + OBSEffect::is_renderable: the region and output size of a rows x cols frame, host only.
 * out_rows = out_cols = 0 selects source x multiplier (cvRound(float(size) * multiplier), half to even); otherwise the output is explicit.
 * crop_ltrb = (left, top, right, bottom) is used iff left + right < cols and top + bottom < rows, else the region is the whole frame.
 * maintain_aspect_ratio: s = min(out_cols / w, out_rows / h) in float, output = cvRound(w s) x cvRound(h s).  Each output dimension is then
 * capped at 4096.  *skip = 1 when an output dimension is <= 0, or when output == frame size and the region is the whole frame: the filter
 * passes such a frame through unchanged.  LVK_HIP_ERR_ARG: rows or cols <= 0, a negative out size, a crop outside [0, 4096], a multiplier
 * that is not > 0 (when used), a NULL pointer. */
int  lvk_hip_fsr_geometry(int rows, int cols, int out_rows, int out_cols, float multiplier, int maintain_aspect_ratio, const int crop_ltrb[4],
                          int region_xywh[4], int out_rows_cols[2], int* skip);
/* The box lvk_hip_draw_text draws into, host only (cv::getTextSize's place): wh = ((6 n - 1) scale + 2 g, 7 scale + 2 g) for n bytes and
 * g = (thickness - 1) / 2, width 0 for an empty string; its top-left corner lies at (x - g, y - 7 scale - g).  *baseline = scale + g: what the
 * cell keeps below y.  Refused like lvk_hip_draw_text, and for a NULL pointer. */
int  lvk_hip_text_size(const char* text, int scale, int thickness, int wh[2], int* baseline);


/* =====================================================================================================================================
 * PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise: per-stage entry points of the parity tests, taps, profiling, device look-ahead)
 * ===================================================================================================================================== */

/* Look-ahead for DEVICE-resident frames, for callers that hold the next frame already (VideoFilter::stream's reader thread runs ahead of
 * its filter thread, Filters/VideoFilter.cpp:62-209; a transcoder whose clip is resident): announce frame n + 1, then push frame n.  The
 * push puts the luma downscale and the pyramid of frame n + 1 on the tracking stream behind its own chain, where the GPU runs them during
 * the host's turn, and the push of frame n + 1 starts at the optical flow.  Only the luma is read ahead (Y plane; channel 0 / the grey
 * value of a packed frame); it must not change between the announcement and the return of the push that carries it.  The announcement
 * holds for the very next push only; a push that carries other planes or another geometry, or that does not track, works as if nothing
 * had been announced.  Same pixels either way.  lvk_hip_stab_prefetch_cancel / lvk_hip_stab_restart forget it.
 * lvk_hip_stab_lookahead_frames: the pushes so far that found their pyramid built. */
int  lvk_hip_stab_prefetch(lvk_hip_stab* stab, const void* d_frame, int step, int rows, int cols, int format);
int  lvk_hip_stab_prefetch_yuv420(lvk_hip_stab* stab, const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step,
                                  int nv12, int rows, int cols);
long long lvk_hip_stab_lookahead_frames(lvk_hip_stab* stab);

/* ---- one-channel (8UC1, LVK_FORMAT_GRAY) frames: what FrameIngest makes of Y800, a monochrome or IR camera ---------------------------------------
 * The reference's lvk::remap asserts CV_8UC3 (Functions/Image.cpp:32); the algorithm does not need three channels.  DEFINITION:
 * the reference's non-YUV EASU program reads the luma of its edge analysis as channel 0 of the pixel, so its twelve tap weights depend on channel 0
 * alone, and each channel is accumulated, normalised, clamped and converted on its own.  The remap of a one-channel frame g is channel 0 of that
 * program run on the three-channel frame (g, c, c) for any constant c, with background (bg, *, *); border, nearest-neighbour and background rules
 * unchanged.  Bit-identical to channel 0 of the three-channel entry with yuv = 0 on (g, c, c).
 * The five entries mirror their three-channel namesakes of PART 1 (same arguments, same refusals, step >= cols) with ONE background byte and no
 * `yuv` argument; in addition source and destination byte ranges that overlap are refused (LVK_HIP_ERR_ARG, the destination untouched).  Any pitch
 * and any byte alignment of either frame.  A 2 x 2 mesh goes through cv::getPerspectiveTransform and the homography kernel. */
int lvk_hip_remap_homography_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                                  void* d_dst, int dst_step, int dst_rows, int dst_cols, int off_x, int off_y, const float H[9], uint8_t bg);
int lvk_hip_remap_mesh_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols, void* d_dst, int dst_step,
                            const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg);
int lvk_hip_remap_map_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                           const void* d_map, int map_step, uint8_t bg);
int lvk_hip_warpmesh_apply_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg);
int lvk_hip_warpmesh_apply_lens_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                     const float* mesh, int mesh_rows, int mesh_cols, uint8_t bg, const lvk_camera_params* lens);
/* The stabilization filter on one-channel device frames: the contract of the packed-frame push of PART 1 (borrowed frame, *released, overlap mode, the
 * DELAYED frame emitted at its own size into a d_out of out_rows rows of out_step >= cols bytes, a push whose output would not fit refused before
 * anything changes) with step >= cols and format LVK_FORMAT_GRAY throughout.  The tracker reads the frame as its own luma; the remap is the
 * one-channel one above with background[0].  The next-output query of PART 1 reports the delayed frame with format LVK_FORMAT_GRAY: one byte per pixel.
 * ONE FORMAT CLASS PER STREAM: a queue that holds three-channel frames refuses a GRAY push, and a queue that holds GRAY frames refuses every
 * three-channel push, with LVK_HIP_ERR_ARG before anything changes; lvk_hip_stab_restart recovers.  The three-channel entries keep refusing
 * LVK_FORMAT_GRAY / Y800 themselves.  The test-mode overlays (draw_trackers, draw_motion_mesh) draw three bytes per pixel and are refused on a GRAY
 * queue; stable_region, stabilize_output = 0 and crop_to_stable_region work as for three channels.  Look-ahead is out of scope for GRAY. */
int  lvk_hip_stab_push_gray(lvk_hip_stab* stab, const void* d_frame, int step, int rows, int cols, uint64_t timestamp,
                            void* d_out, int out_step, int out_rows, int* produced, uint64_t* out_timestamp, const void** released,
                            lvk_frame_info* emitted);
/* The same push for a frame in PINNED host memory, one plane each way: h_frame is uploaded on the filter's upload stream into a block the library owns
 * until that frame has been emitted (the host plane is the caller's again when the call returns), and the one-channel remap stores the emitted frame
 * straight into oh_out, a pinned plane of out_rows rows of out_step >= cols bytes (complete after lvk_hip_sync).  Size rule, format class, overlap mode
 * as above.  Refused with LVK_HIP_ERR_ARG before anything is uploaded or queued: everything lvk_hip_stab_push_gray refuses, a pageable input or output
 * plane (either end of its extent), frames borrowed by lvk_hip_stab_push_gray still queued (and the reverse: the two do not share a queue;
 * lvk_hip_stab_restart recovers), and a push while frames announced through lvk_hip_stab_prefetch_yuv420_host are outstanding. */
int  lvk_hip_stab_push_gray_host(lvk_hip_stab* stab, const void* h_frame, int step, int rows, int cols, uint64_t timestamp,
                                 void* oh_out, int out_step, int out_rows, int* produced, uint64_t* out_timestamp, lvk_frame_info* emitted);

/* ---- four-channel (8UC4, LVK_FORMAT_BGRA / LVK_FORMAT_RGBA) frames: what game, window and display captures and every source with transparency hand over;
 * BGRX is a BGRA frame whose fourth byte is carried like alpha ---------------------------------------------------------------------------------------
 * DEFINITION: in the reference's non-YUV EASU program the twelve tap weights depend on channel 0 alone and each channel is
 * accumulated, normalised, clamped and converted on its own, so output channel k depends on input channels 0 and k only.  The remap of a four-channel
 * frame (c0, c1, c2, a) with background (b0, b1, b2, b3) is that program with a fourth channel under the same weights: bytes 0 .. 2 are bit-identical to
 * the three-channel entry with yuv = 0 on (c0, c1, c2) and background (b0, b1, b2), byte 3 to channel 1 of the three-channel entry with yuv = 0 on
 * (c0, a, a) and background (b0, b3, b3).  Border, nearest-neighbour (all four bytes copied) and background rules unchanged.  The same for BGRA and RGBA:
 * the program does not know which of channels 0 and 2 is red.  There is no four-channel YUV format.
 * The five entries mirror their `_gray` namesakes with FOUR background bytes.  Both frames are 4-byte aligned, both pitches multiples of 4, step >=
 * 4 * cols, source and destination byte ranges do not overlap: anything else is refused with LVK_HIP_ERR_ARG, the destination untouched.  The kernels are
 * exact in both remap precisions (no LVK_REMAP_1LSB twins).  A 2 x 2 mesh goes through cv::getPerspectiveTransform and the homography kernel. */
int lvk_hip_remap_homography_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols,
                                void* d_dst, int dst_step, int dst_rows, int dst_cols, int off_x, int off_y, const float H[9], const uint8_t bg[4]);
int lvk_hip_remap_mesh_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols, void* d_dst, int dst_step,
                          const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4]);
int lvk_hip_remap_map_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                         const void* d_map, int map_step, const uint8_t bg[4]);
int lvk_hip_warpmesh_apply_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                              const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4]);
int lvk_hip_warpmesh_apply_lens_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step,
                                   const float* mesh, int mesh_rows, int mesh_cols, const uint8_t bg[4], const lvk_camera_params* lens);
/* The stabilization filter on four-channel device frames: the contract of the packed-frame push of PART 1 (borrowed frame, *released, overlap mode and
 * persistent grid, the DELAYED frame emitted at its own size into a d_out of out_rows rows of out_step >= 4 * cols bytes, a push whose output would not
 * fit refused before anything changes).  format is LVK_FORMAT_BGRA or LVK_FORMAT_RGBA; frame and output are 4-byte aligned with pitches that are multiples
 * of 4.  The tracker reads cvtColor(..2GRAY) of the colour bytes; the remap is the four-channel one above with background_colour[0..3]: [0..2] are
 * lvk_stab_settings::background, whose layout is fixed, and [3] is set by lvk_hip_stab_set_background_alpha (0 .. 255; 0 when never set, the fourth value
 * of the reference's three-value cv::Scalar default; kept across configure()).  The next-output query of PART 1 reports the delayed frame with its own
 * format: four bytes per pixel.
 * ONE PIXEL SIZE PER STREAM: a queue holds frames of 1, 3 or 4 bytes per pixel, and every push of another size -- through any entry -- is refused with
 * LVK_HIP_ERR_ARG before anything changes; so is an RGBA push into a BGRA queue and the reverse.  lvk_hip_stab_restart recovers.  The three-channel entries
 * keep refusing LVK_FORMAT_BGRA / LVK_FORMAT_RGBA themselves, and lvk_hip_stab_push_obs / _obs_host keep DirectIngest's route for RGBA / BGRA / BGRX.
 * DECLARED GAPS: the test-mode overlays (draw_trackers, draw_motion_mesh) draw three bytes per pixel and are refused on a four-channel queue; there is
 * no look-ahead / prefetch for four-channel frames.  stable_region, stabilize_output = 0 and crop_to_stable_region work as for three channels. */
int  lvk_hip_stab_set_background_alpha(lvk_hip_stab* stab, int alpha);
int  lvk_hip_stab_push_c4(lvk_hip_stab* stab, const void* d_frame, int step, int rows, int cols, uint64_t timestamp, int format,
                          void* d_out, int out_step, int out_rows, int* produced, uint64_t* out_timestamp, const void** released,
                          lvk_frame_info* emitted);
/* The same push for a frame in PINNED host memory, one plane each way, built as lvk_hip_stab_push_gray_host is: h_frame (any alignment, step >= 4 * cols)
 * goes up in one copy into a block the library owns until that frame has been emitted, and the four-channel remap stores the emitted frame straight into
 * oh_out, a pinned plane of out_rows rows of out_step >= 4 * cols bytes, 4-byte aligned, out_step a multiple of 4 (complete after lvk_hip_sync).  Refused
 * with LVK_HIP_ERR_ARG before anything is uploaded or queued: everything lvk_hip_stab_push_c4 refuses, a pageable input or output plane, frames borrowed
 * by lvk_hip_stab_push_c4 still queued (and the reverse), and a push while frames announced through lvk_hip_stab_prefetch_yuv420_host are outstanding. */
int  lvk_hip_stab_push_c4_host(lvk_hip_stab* stab, const void* h_frame, int step, int rows, int cols, uint64_t timestamp, int format,
                               void* oh_out, int out_step, int out_rows, int* produced, uint64_t* out_timestamp, lvk_frame_info* emitted);

/* ---- lvk::ScalingFilter on one- and four-channel frames: EASU upscale and RCAS of what the GRAY and four-channel pushes above emit --------------------
 * The reference's lvk::upscale and lvk::sharpen assert CV_8UC3 (Functions/Image.cpp:159,208).  DEFINITIONS, each through the
 * three-channel program of PART 1:
 *   upscale, GRAY: channel 0 of lvk_hip_upscale with yuv = 0 (the easu_scale program whose luma is channel 0) on (g, c, c), for any constant c;
 *   upscale, four channels (c0, c1, c2, a): bytes 0 .. 2 are lvk_hip_upscale with yuv = 0 on (c0, c1, c2), byte 3 is its channel 1 on (c0, a, a) -- the alpha
 *     is resampled under the colour's weights, as in the four-channel remaps.  No `yuv` argument: there is no four-channel YUV format, and
 *     ScalingFilterSettings::yuv_input is ignored for these frames;
 *   sharpen, GRAY: any channel of lvk_hip_sharpen on (g, g, g) -- the rcas program with one channel, lobe = min(max(lobe_0, -0.1875), 0) * sharp; a NaN
 *     limiter (0 x inf at a saturated ring) loses against -0.1875;
 *   sharpen, four channels: bytes 0 .. 2 are lvk_hip_sharpen on (c0, c1, c2), byte 3 is the SOURCE pixel's alpha, copied: the limiter is built from the
 *     colour channels and bounds only them, so a lobe applied to alpha could leave [0, 1] and wrap in the truncating conversion, and alpha cannot join the
 *     limiter, whose three lobes are coupled through their maximum, without changing the colours.  Border pixels are copied, alpha included.
 * All four are asynchronous on the context's stream, out of place and exact in every remap precision.  Refused with LVK_HIP_ERR_ARG, the destination
 * untouched: a NULL pointer, rows or cols <= 0, a step below BPP * cols, a destination smaller than the source in either dimension (upscale; the same size
 * copies), sharpness outside [0, 1] or NaN, source and destination byte ranges that overlap, and for `_c4` a base or pitch that is not a multiple of 4.
 * `_gray` takes any base address and any pitch. */
int lvk_hip_upscale_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols, void* d_dst, int dst_step, int dst_rows, int dst_cols);
int lvk_hip_upscale_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int src_rows, int src_cols, void* d_dst, int dst_step, int dst_rows, int dst_cols);
int lvk_hip_sharpen_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step, float sharpness);
int lvk_hip_sharpen_c4(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step, float sharpness);

/* ---- lvk::CASFilter and lvk::FSRFilter on one-channel frames ------------------------------------------------------------------------------------------
 * The plugin runs both filters as RGBA effects: there is no one-channel program.  DEFINITIONS, each through the three-channel
 * specification of PART 1's entry, which keeps refusing LVK_FORMAT_GRAY itself:
 *   CAS, GRAY: channel 0 of the three-channel CAS on (g, g, g) -- CAS sharpens every channel on its own, so this is the program with one channel; neighbours
 *     outside the frame read as 0, the load is the correctly rounded u / 255, the store rint(v * 255);
 *   EASU, GRAY: channel 0 of the three-channel EASU on (g, g, g), the same for BGR, RGB and YUV; region_xywh, the clamp-to-edge taps and the output size are
 *     those of the three-channel entry, and the geometry call of PART 1 serves both.
 * Both are asynchronous on the context's stream and out of place, at any base address and any pitch.  Refused with LVK_HIP_ERR_ARG, the destination
 * untouched: a NULL pointer, a size <= 0, a step below its row, sharpness outside [0, 1] or NaN, an empty region or one outside the frame, source and
 * destination byte ranges that overlap. */
int lvk_hip_cas_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step, float sharpness);
int lvk_hip_fsr_easu_gray(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, const int region_xywh[4],
                          void* d_dst, int dst_step, int out_rows, int out_cols);
/* The kernel path lvk_hip_fsr_easu_gray takes for a rw x rh region scaled to out_rows x out_cols: 0 = staged, 1 = direct (a one-channel texel is a
 * quarter of a staged three-channel one, so more scales stay staged); LVK_HIP_ERR_ARG for a size <= 0.  Host only, for the tests. */
int lvk_hip_fsr_easu_gray_path(int rw, int rh, int out_rows, int out_cols);

/* ---- lvk::DeblockingFilter on one- and four-channel frames ------------------------------------------------------------------------------------------
 * The GRAY and BGRA / RGBA forms of lvk_hip_deblock_apply, on the same handle, are declared in lvk_hip_deblock_px.h, which this header includes at its
 * end: a host that includes lvk_hip.h sees them like every other entry of PART 2. */

/* Which schedule the pushes of this filter took so far.  The library picks per push, from what it sees the caller doing (is the bulk stream still
 * busy with the previous remap? did this push begin within 15 us of the last one's return?), between the schedule of a FREE-RUNNING caller
 * (persistent remap grid of 4 blocks per CU next to the tracker, completion through an event) and that of a caller that WAITS for every frame
 * (full remap grid, completion through a word in host memory): same pixels, different throughput / latency.  (After eight or more free-running pushes
 * the first push that looks synchronous still takes the free-running schedule -- one synchronisation does not make a synchronous caller --, the second
 * in a row switches.)  A host -- and bench.py, per leg --
 * reads here which one its pushes got.  reset != 0 zeroes the counters after reading. */
#define LVK_SCHED_PUSH_FREE_RUNNING   0   /* pushes taken as a free-running caller's ... */
#define LVK_SCHED_PUSH_SYNCHRONISED   1   /* ... and as those of a caller that waits for every frame */
#define LVK_SCHED_INGEST_ON_TRACKER   2   /* 4:2:0 conversions placed behind the chain on the tracking stream ... */
#define LVK_SCHED_INGEST_ON_BULK      3   /* ... on the bulk stream (overlap mode) ... */
#define LVK_SCHED_INGEST_INLINE       4   /* ... ahead of the tracker on the context's stream (no overlap) */
#define LVK_SCHED_REMAP_PERSISTENT    5   /* output remaps launched as the persistent co-scheduled grid ... */
#define LVK_SCHED_REMAP_FULL          6   /* ... as the full grid */
#define LVK_SCHED_WAIT_SIGNAL_WORD    7   /* chain completions taken from the host signal word ... */
#define LVK_SCHED_WAIT_EVENT          8   /* ... from hipEventSynchronize / hipStreamSynchronize */
#define LVK_SCHED_WAIT_WORD_TIMEOUT   9   /* signal-word waits that fell through to the event / stream wait (bounded spin) */
#define LVK_SCHED_COUNT              10
int  lvk_hip_stab_schedule_counters(lvk_hip_stab* stab, long long out[LVK_SCHED_COUNT], int reset);

int  lvk_hip_stab_get_stats(const lvk_hip_stab* stab, lvk_stab_stats* out);
/* Frames on which FeatureDetector::detect ran FAST so far (Vision/FeatureDetector.cpp:125-157), by where the corners went through the
 * suppression grid: on the device inside the tracker's chain of kernels, or in the host loop (grids beyond 4096 cells, detection regions off
 * the pixel grid, LVK_HIP_HOST_GRID=1).  Same features either way; a tap for tests and tuning. */
int  lvk_hip_stab_detector_frames(const lvk_hip_stab* stab, long long* on_device, long long* on_host);
/* last frame motion (after the trust factor) and last applied correction; each motion_height x motion_width x 2 floats */
int  lvk_hip_stab_get_meshes(const lvk_hip_stab* stab, float* motion, float* correction, int cap_floats);
/* FrameTracker::features(): (x, y, response, age) per tracked feature; returns the total count */
int  lvk_hip_stab_get_features(const lvk_hip_stab* stab, float* xy_resp_age, int cap);


/* ---- timing (reference: VideoFilter::timings() / Stopwatch::sync_gpu, Filters/VideoFilter.cpp:46-51) ---------
 * Per-stage GPU time from HIP events recorded on the launch stream around each stage's kernels. */
#define LVK_STAGE_DOWNSCALE 0   /* luma + INTER_AREA */
#define LVK_STAGE_PYRAMID   1   /* pyrDown x3 + Scharr x4 */
#define LVK_STAGE_FAST      2   /* FAST-9/16 + NMS + compaction */
#define LVK_STAGE_PYRLK     3   /* sparse optical flow */
#define LVK_STAGE_MOTION    4   /* RANSAC + local optimisation */
#define LVK_STAGE_REMAP     5   /* EASU remap of the delayed frame */
#define LVK_STAGE_INGEST    6   /* YUV420 -> packed 444 (lvk_hip_stab_push_yuv420 only) */
#define LVK_STAGE_EGRESS    7   /* packed 444 -> YUV420 */
#define LVK_STAGE_COUNT     8
/* enable: 0 = off, 1 = every stage, otherwise a set of (1 << (LVK_STAGE_x + 1)) bits -- each timed stage costs two event records
 * per frame on the host, so a measurement that needs one kernel should ask for that stage only; bits 16..23 = N: time the stages
 * of one push in N only (0 / 1 = every push), which keeps a live measurement from slowing the stream it measures */
int  lvk_hip_stab_set_profiling(lvk_hip_stab* stab, int enable);
int  lvk_hip_stab_get_profile(lvk_hip_stab* stab, double total_ms[LVK_STAGE_COUNT], long long launches[LVK_STAGE_COUNT]);

/* native_recip(x) of FSR.cl as the EASU / RCAS kernels of this library evaluate it (v_rcp_f32, what the reference's OpenCL source
 * compiles to for gfx950), elementwise over n binary32 values on the device.  OpenCL leaves native_recip implementation-defined:
 * this entry point lets a host (and the parity tests' CPU model of the kernels) read the device's definition. */
int lvk_hip_native_rcp(lvk_hip_ctx* ctx, const float* d_in, float* d_out, size_t n);

/* ---- a10: local motion estimate (vector-field preset) ---------------------------------------------------------------
 * FrameTracker::estimate_local_motions with the constraint system of generate_mesh_constraints (Vision/FrameTracker.cpp:200-321,
 * 380-457) for a mesh of cols x rows vertices: the least-squares positions of the mesh vertices from the tracked -> matched point pairs
 * (host arrays of n x 2 floats, tracking-frame coordinates), the temporal rows pulling towards the previous solution, which the
 * solver object keeps (the reference's m_OptimizedMesh; _reset zeroes it like FrameTracker::restart).  gen_region / the smoothing
 * weights are those in force when the reference (re)generates the constraints (:74-82); region / temporal_now those of the call.
 * Outputs: inlier flag per pair (L1 reprojection error < threshold) and the cols x rows x 2 normalised backward offsets of the motion
 * mesh.  Returns 0, or 2 / 3 when no estimate is possible (a point in the mesh's last cell row / column, singular system).
 * Solved on the device (normal equations, band L D L^T in binary64).  Any mesh size the remap takes (cols x rows x 8 bytes <= 64 KB,
 * up to 167 columns): meshes up to 16 columns and 2048 unknowns (16 x 64 vertices) run the register-window kernels (the 16 x 16 preset:
 * ~0.2 ms), larger or wider ones (17 x 17, 32 x 32, ...) generic kernels with the same arithmetic and the same bits (milliseconds). */
typedef struct lvk_hip_mesh_solver lvk_hip_mesh_solver;
int  lvk_hip_mesh_solver_create(lvk_hip_ctx* ctx, int cols, int rows, float gen_region_w, float gen_region_h,
                                float temporal_smoothing, float local_smoothing, int max_points, lvk_hip_mesh_solver** out);
void lvk_hip_mesh_solver_destroy(lvk_hip_mesh_solver* solver);
int  lvk_hip_mesh_solver_reset(lvk_hip_mesh_solver* solver);
int  lvk_hip_mesh_solver_solve(lvk_hip_mesh_solver* solver, const float* tracked, const float* matched, int n, float region_w, float region_h,
                               float temporal_now, float threshold, uint8_t* inliers, float* offsets);

/* ---- a3/a4: luma + INTER_AREA downscale ---------------------------------------------------------------
 * VideoFrame::viewAsFormat(GRAY) for YUV frames (= channel 0, Data/VideoFrame.cpp:260) fused with
 * cv::resize(gray, detection_resolution, INTER_AREA) (Vision/FrameTracker.cpp:117).
 * pix_stride = bytes per source pixel (3 packed 8UC3, 1 planar); d_dst is 8UC1 drows x dcols.  Any pair of sizes: integer and fractional
 * reductions, and (a frame smaller than the detection resolution) cv::resize's bilinear emulation of INTER_AREA towards a larger image.
 * LVK_HIP_ERR_ARG, nothing written, for a pitch shorter than its row (src_step < scols * pix_stride, dst_step < dcols), like the remap entries. */
int lvk_hip_luma_area_resize(lvk_hip_ctx* ctx, const void* d_src, int src_step, int pix_stride, int channel,
                             int srows, int scols, void* d_dst, int dst_step, int drows, int dcols);

/* ---- a7 (pyramid): cv::pyrDown and the Scharr derivative image that cv::SparsePyrLKOpticalFlow::calc builds
 * internally (Vision/FrameTracker.cpp:140-146).  d_dst of pyr_down is ((cols+1)/2) x ((rows+1)/2) 8UC1;
 * d_dst of scharr is rows x cols x (Ix, Iy) int16, tightly packed.  LVK_HIP_ERR_ARG, nothing written, for a pitch shorter than its row
 * (src_step < cols; pyr_down: dst_step < (cols + 1) / 2), like the remap entries. */
int lvk_hip_pyr_down(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step);
int lvk_hip_scharr(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, void* d_dst);

/* The whole optical-flow pyramid of buildOpticalFlowPyramid (levels until one would be <= the window) plus every
 * level's Scharr image, returned to the host tightly packed level after level.  Returns the level count.  Synchronous.
 * LVK_HIP_ERR_ARG, nothing written, for step < cols, like the remap entries. */
int lvk_hip_build_pyramid(lvk_hip_ctx* ctx, const void* d_img, int step, int rows, int cols, int max_level, int win_w, int win_h,
                          uint8_t* levels, int16_t* derivs, int* level_rows, int* level_cols);

/* ---- a5 (inner): FAST-9/16 + non-max suppression per detection region -----------------------------------
 * cv::FastFeatureDetector(threshold, true, TYPE_9_16)->detect(frame(region)) (Vision/FeatureDetector.cpp:130-134).
 * regions = nregions x {x, y, w, h, threshold, active} ints; out = nregions x cap keypoints packed as
 * x | y << 12 | score << 24 (region-local, row-major like the CPU detector); counts = nregions totals.
 * Synchronous (returns after the results are on the host).  LVK_HIP_ERR_ARG, nothing written, for step < cols, like the remap entries. */
int lvk_hip_fast_detect(lvk_hip_ctx* ctx, const void* d_img, int step, int rows, int cols,
                        const int* regions, int nregions, uint32_t* out, int cap, int* counts);

/* ---- a7: cv::SparsePyrLKOpticalFlow::calc(prev, next, prevPts, nextPts, status) -----------------------------
 * (Vision/FrameTracker.cpp:42-48,140-146).  Device images of the tracking resolution, host point arrays
 * (n x 2 floats), status n bytes.  Synchronous. */
int lvk_hip_pyrlk(lvk_hip_ctx* ctx, const void* d_prev, int prev_step, const void* d_next, int next_step, int rows, int cols,
                  const float* prev_pts, int n, float* next_pts, uint8_t* status,
                  int win_w, int win_h, int max_level, int max_count, double epsilon, double min_eig_threshold);

/* ---- a9: robust global motion --------------------------------------------------------------------------
 * cv::findHomography(tracked, matched, mask, UsacParams{threshold}) (full_homography != 0) or
 * cv::estimateAffinePartial2D(..., RANSAC, threshold, 50) + Homography::FromAffineMatrix (full_homography == 0)
 * as used by FrameTracker::estimate_global_motion (Vision/FrameTracker.cpp:325-375).  Host point arrays (n x 2
 * floats); H = 3x3 row-major double normalised by H22; mask = n bytes.  (region_w, region_h) = tracking resolution.
 * Returns the inlier count, or a negative value when no model exists (H = identity, mask = 0).  Synchronous.
 * The estimator is the deterministic RANSAC of DESIGN.md (OpenCV's USAC is randomised and not restated). */
int lvk_hip_estimate_global_motion(lvk_hip_ctx* ctx, const float* pts1, const float* pts2, int n, double threshold,
                                   double region_w, double region_h, int full_homography, double H[9], uint8_t* mask);

/* The same estimate with the mode of its local optimisation chosen by the caller, and what the kernel reports of it.
 *   lo_mode 0   what lvk_hip_estimate_global_motion, the chain and the filter run: the refit rounds stop at a mask fixed point -- after an
 *               accepted round whose inlier mask equals the mask its refit was computed on, the next round would repeat it bit for bit
 *               and change nothing.
 *   lo_mode 1   every round the loop of the specification runs.  Same H, mask and return value, by construction.
 * lo_info[0] = refit rounds executed, lo_info[1] = 1 when the loop was left at a fixed point with a round still to go (0 in mode 1, and 0, 0
 * where no kernel ran).  Synchronous; a test entry. */
int lvk_hip_estimate_global_motion_lo(lvk_hip_ctx* ctx, const float* pts1, const float* pts2, int n, double threshold,
                                      double region_w, double region_h, int full_homography, int lo_mode, double H[9], uint8_t* mask,
                                      int lo_info[2]);

/* fast_filter (Functions/Container.tpp:97-121; call site Vision/FrameTracker.cpp:149) as the GPU runs it between the optical
 * flow and the motion estimate: keeps the pairs whose status is non-zero, in the order the reference's back-to-front swap-erase
 * leaves them.  Host arrays (n x 2 floats, n bytes); returns the number of pairs kept (>= 0) or LVK_HIP_ERR_*. */
int lvk_hip_fast_filter(lvk_hip_ctx* ctx, const float* prev, const float* matched, const uint8_t* status, int n, float* out_prev, float* out_matched);

/* The tracker's chain optical flow -> fast_filter -> robust global motion (Vision/FrameTracker.cpp:140-168, 325-375) through the SAME launcher
 * the stabilization filter enqueues it with, in a variant the caller selects; synchronous, per-call allocations (a test entry).
 *   start       d_prev_img == NULL: from a flow result -- prev / matched (n_bound x 2 floats), status (n_bound bytes) and optionally und, the
 *               lens-corrected positions (previous | matched), 2 x n_eff x 2 floats with n_eff = the effective count (below).
 *               d_prev_img != NULL: from two device images (rows x cols, 8UC1) and prev: the flow kernel runs in its chained form (points read
 *               from pinned host memory; with `lens` -- a profile for a lens_rows x lens_cols frame, lens_sx / lens_sy = frame / tracking size --
 *               it writes the corrected positions itself).
 *   compaction  separate_compact == 0: as the filter decides (inside the RANSAC's first kernel up to 2048 points, a kernel of its own beyond);
 *               != 0: a kernel of its own for any n_bound.
 *   count       count_on_device == 0: n_bound points.  != 0: the kernels read n_word from device memory and clamp it to [0, n_bound]
 *               (n_eff); n_bound is the launch bound.
 *   model       model_on_device == 0: `full` (homography / similarity).  != 0: the kernels read full_word from device memory, `full` is ignored.
 *   completion  host_signal == 0: stream synchronisation.  != 0: the last kernel stores a word in host memory and the entry reads H, the
 *               code, the mask and the host mirrors once it has seen it, as the filter does (signalled = 1; 0: the word came late).
 * Results: H, rc (inlier count, or -12: no model -- fewer pairs than the model needs included, the count being the device's); mask (n_bound
 * bytes, the first count meaningful); pairs_dev = the compacted pairs in device memory (p1 | p2, 2 x n_bound x 2 floats) and count_dev;
 * count_host, mirror_matched, mirror_status = the host mirrors; when the flow ran, next_pts / flow_status (n_bound + 2 GUARD entries) and
 * flow_und (2 n_bound + 2 GUARD entries; may be NULL without `lens`): the kernel's output buffers with GUARD entries in front and behind.
 * Every output byte no kernel wrote holds LVK_TRACK_CHAIN_FILL. */
#define LVK_TRACK_CHAIN_GUARD 64
#define LVK_TRACK_CHAIN_FILL  0xA5
typedef struct lvk_track_chain_desc
{
    const float* prev; const float* matched; const uint8_t* status; const float* und;
    const void* d_prev_img; int prev_step; const void* d_next_img; int next_step; int rows, cols;
    int win_w, win_h, max_level, max_count; double epsilon, min_eig;
    const lvk_camera_params* lens; int lens_rows, lens_cols; double lens_sx, lens_sy;
    int n_bound, count_on_device, n_word;
    int full, model_on_device, full_word;
    int separate_compact, host_signal;
    double threshold; int region_w, region_h;
} lvk_track_chain_desc;
typedef struct lvk_track_chain_result
{
    double H[9]; int rc, signalled, count_dev, count_host;
    uint8_t* mask; float* pairs_dev; float* mirror_matched; uint8_t* mirror_status;
    float* next_pts; uint8_t* flow_status; float* flow_und;
} lvk_track_chain_result;
int lvk_hip_track_chain(lvk_hip_ctx* ctx, const lvk_track_chain_desc* desc, lvk_track_chain_result* result);

/* Deblocking tap: the block grids of the last apply (synchronises the context's stream).  mean = the 8U block means, grid = the 8U mean absolute
 * deviations from them, keep_block = float(min(grid, L) * (1.0 / L)); ex * ey values each, row-major (NULL: skipped).  extent_xy = (ex, ey).
 * Returns ex * ey, or LVK_HIP_ERR_ARG before the first apply or when capacity < ex * ey. */
int lvk_hip_deblock_get_grid(lvk_hip_deblock* deb, uint8_t* mean, uint8_t* grid, float* keep_block, int capacity, int extent_xy[2]);

/* The deblocking filter on the planes of an I420 / NV12 frame in one call, lvk_hip_deblock_apply_yuv420 on the same handle, is declared in
 * lvk_hip_deblock_420.h, which this header includes at its end like lvk_hip_deblock_px.h; the same on the planes of every OBS video format,
 * lvk_hip_deblock_apply_obs, in lvk_hip_deblock_obs.h, which that header includes. */

/* CAS host constant (CasSetup's const1.x, float32, each operation rounded on its own): peak = -(1 / (5 s + ((-8) s + 8))) with
 * s = clamp(sharpness, 0, 1).  Needs no device.  LVK_HIP_ERR_ARG for a NaN sharpness or a NULL peak. */
int lvk_hip_cas_const(float sharpness, float* peak);

/* ConversionFilter's table (Filters/ConversionFilter.cpp:46-57): the LVK_FORMAT_* that cvtColor(code, dcn) makes of a src_format frame, or -1
 * when the combination is refused.  Codes (OpenCV's values): BGR2BGRA 0 (= RGB2RGBA), BGRA2BGR 1, BGR2RGBA 2, RGBA2BGR 3, BGR2RGB 4,
 * BGRA2RGBA 5, BGR2GRAY 6, RGB2GRAY 7, GRAY2BGR 8, GRAY2BGRA 9, BGRA2GRAY 10, RGBA2GRAY 11, BGR2YUV 82, RGB2YUV 83, YUV2BGR 84, YUV2RGB 85;
 * any other code is refused.  An aliased code takes both of its source formats; BGR2YUV / RGB2YUV and the *2GRAY codes also take the frame
 * of the same channel order with the other channel count (OpenCV's scn = 3 or 4).  dcn is 0 or the code's destination channel count;
 * YUV2BGR / YUV2RGB also take dcn 4 (BGRA / RGBA).  Needs no device. */
int lvk_hip_cvt_code_target(int code, int src_format, int dcn);

/* FSR host constants (FsrEasuCon on the CPU, float32, each operation rounded on its own, rcp = 1 / x): con[0..15] = con0 .. con3 for a
 * rw x rh viewport of a W x H input scaled to ow x oh.  Needs no device.  LVK_HIP_ERR_ARG for a size <= 0 or a NULL con. */
int lvk_hip_fsr_easu_const(int rw, int rh, int W, int H, int ow, int oh, float con[16]);

/* The kernel path lvk_hip_fsr_easu takes for a rw x rh region scaled to out_rows x out_cols: 0 = staged (the tile's source footprint in
 * LDS), 1 = direct (taps read from the frame; downscales whose footprint does not fit).  Needs no device.  LVK_HIP_ERR_ARG for a size <= 0. */
int lvk_hip_fsr_easu_path(int rw, int rh, int out_rows, int out_cols);

/* The kernel form lvk_hip_luma_area_resize (and the stabilizer's tracking-frame downscale, the same launcher) runs for these arguments: one
 * value per form, chosen by the exactness of the scale, the pixel stride, the channel, the tap count per axis and the alignment of the
 * source base and pitch.  FAST_DW_<sx>x<sy>_<source>: the dword-load kernels for 4-byte aligned planes (C3 = packed three-byte pixels,
 * channel 0 / BGR -> gray / RGB -> gray; C1 = planar); FAST: any other integer scale; TILE_<n> (planar, LDS window) and TAPS_<n> (one channel
 * of packed pixels): fractional scales with up to n taps per axis; GENERAL: the tap loops; ENLARGE: a destination larger on either axis.
 * Launches nothing (a fractional scale stages its tap tables in the context, as the resize itself would).  Returns the form, or
 * LVK_HIP_ERR_* for arguments the resize refuses. */
enum
{
    LVK_AREA_PATH_FAST_DW_8x8_C3_BGR = 0, LVK_AREA_PATH_FAST_DW_8x8_C3_RGB = 1, LVK_AREA_PATH_FAST_DW_4x4_C3_BGR = 2, LVK_AREA_PATH_FAST_DW_4x4_C3_RGB = 3,
    LVK_AREA_PATH_FAST_DW_8x8_C3 = 4, LVK_AREA_PATH_FAST_DW_4x4_C3 = 5, LVK_AREA_PATH_FAST_DW_8x8_C1 = 6, LVK_AREA_PATH_FAST_DW_4x4_C1 = 7,
    LVK_AREA_PATH_FAST = 8, LVK_AREA_PATH_TILE_4 = 9, LVK_AREA_PATH_TILE_8 = 10, LVK_AREA_PATH_TAPS_4 = 11, LVK_AREA_PATH_TAPS_8 = 12,
    LVK_AREA_PATH_GENERAL = 13, LVK_AREA_PATH_ENLARGE = 14, LVK_AREA_PATH_COUNT = 15
};
int lvk_hip_area_resize_path(lvk_hip_ctx* ctx, const void* d_src, int src_step, int pix_stride, int channel,
                             int srows, int scols, int drows, int dcols);

/* ---- lvk::LCFilter: the OBS plugin's lens correction (Modules/OBS-Plugin/Sources/Enhancement/LCFilter.cpp:133-192) as an object ---------------------
 * DESIGN.md section 27.  First the one primitive it adds, the counterpart of lvk_hip_warpmesh_apply_yuv420 for a materialised map: d_src is a packed YUV
 * 8UC3 frame, d_map a rows x cols float2 offset map in pixels (what lvk_hip_lens_map_create builds; 8-byte aligned, map_step a multiple of 8), the output
 * I420 (o_y, o_u, o_v) or NV12 (o_y, o_u = the UV plane, o_v ignored) planes: byte for byte lvk_hip_remap_map(.., yuv = 1) followed by
 * lvk_hip_egress_yuv420, in one kernel, in the context's remap precision.  Asynchronous on the context's stream.  Refused with LVK_HIP_ERR_ARG, nothing
 * written: a NULL pointer that is in use, odd rows or cols or either below 2, a pitch below its row, a map lvk_hip_remap_map refuses, the source's or the
 * map's byte range overlapping an output plane, two output planes overlapping. */
int lvk_hip_remap_map_yuv420(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols,
                             void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int nv12,
                             const void* d_map, int map_step, const uint8_t bg[3]);
/* The filter.  It owns the camera profile (NULL: none selected -- frames pass through), the offset map of the LAST frame size -- built at the first apply,
 * again when the frame size or the profile changed (`m_MeshOutdated || size != frame.size()`), the old map released behind the stream -- and the test
 * mode: lvk::draw_grid(frame, {32, 32}, col::MAGENTA[format], 1), (105, 212, 234) on YUV and (255, 0, 255) on BGR / RGB frames, drawn BEFORE the warp and
 * warped with the frame.  Background (0, 0, 0[, 0]), WarpMesh::apply's default; the YUV EASU program for LVK_FORMAT_YUV, the RGB one otherwise.  Applies
 * are asynchronous on the context's stream and out of place (overlapping source and destination are refused); the map build is synchronous host work.
 *   _configure         a profile with fx == 0 or fy == 0 is refused and leaves the object as it was (so does _create: no object).
 *   _view              the valid-pixel region of cv::getOptimalNewCameraMatrix (x, y, w, h) for a rows x cols frame; the whole frame without a profile.
 *   _apply             three channels (LVK_FORMAT_BGR, _RGB, _YUV): [lvk_hip_draw_grid into d_src] -> lvk_hip_remap_map(d_src -> d_dst); a copy without a
 *                      profile.  IN TEST MODE THE GRID IS DRAWN INTO THE CALLER'S SOURCE FRAME, as the reference draws into the frame it is handed;
 *                      outside test mode d_src is not written.
 *   _apply_gray / _c4  lvk_hip_remap_map_gray / _c4 (LVK_FORMAT_BGRA, _RGBA) with the same map; a copy without a profile.  DECLARED GAP: the grid kernel
 *                      writes three bytes per pixel, so both are refused in test mode (LVK_HIP_ERR_ARG, nothing written), like the stabilizer's overlays.
 *   _apply_yuv420      I420 / NV12 planes in, planes out (NV12: d_u / o_u are the UV planes, d_v / o_v ignored): byte for byte lvk_hip_ingest_yuv420 ->
 *                      [lvk_hip_draw_grid, YUV magenta] -> lvk_hip_remap_map(yuv = 1, bg 0, 0, 0) -> lvk_hip_egress_yuv420, the remap and the egress as one
 *                      kernel; without a profile ingest -> [grid] -> egress (the chroma is the up- and down-sampled chroma, as in the plugin).  The packed
 *                      frame in between is a block of the context's pool that returns to it inside the call; the input planes are never written.
 *                      Refused with LVK_HIP_ERR_ARG, nothing written or enqueued: a NULL plane that is in use, odd rows or cols or either below 2, a pitch
 *                      below its row, an input plane overlapping an output plane, two output planes overlapping.
 * A NULL object is refused.  The object must be destroyed before its context. */
typedef struct lvk_hip_lens lvk_hip_lens;
int  lvk_hip_lens_create(lvk_hip_ctx* ctx, const lvk_camera_params* profile /* NULL: none selected */, int test_mode, lvk_hip_lens** out);
int  lvk_hip_lens_configure(lvk_hip_lens* lens, const lvk_camera_params* profile, int test_mode);
void lvk_hip_lens_destroy(lvk_hip_lens* lens);
int  lvk_hip_lens_view(lvk_hip_lens* lens, int rows, int cols, int view_xywh[4]);
int  lvk_hip_lens_apply(lvk_hip_lens* lens, void* d_src, int src_step, int rows, int cols, int format, void* d_dst, int dst_step);
int  lvk_hip_lens_apply_gray(lvk_hip_lens* lens, const void* d_src, int src_step, int rows, int cols, void* d_dst, int dst_step);
int  lvk_hip_lens_apply_c4(lvk_hip_lens* lens, const void* d_src, int src_step, int rows, int cols, int format, void* d_dst, int dst_step);
int  lvk_hip_lens_apply_yuv420(lvk_hip_lens* lens, const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step,
                               void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int rows, int cols, int nv12);

/* ---- the same for EVERY video format FrameIngest::Select accepts ------------------------------------------------------------------
 * lvk_hip_remap_map_obs: the primitive.  d_src a packed YUV 8UC3 frame, d_map as for lvk_hip_remap_map_yuv420, o_planes / o_steps the planes of
 * `video_format` as lvk_hip_egress_obs takes them: byte for byte lvk_hip_remap_map(.., yuv = 1) followed by lvk_hip_egress_obs, in one kernel, in the
 * context's remap precision.  It takes I422 / I42A, YUY2 / YVYU / UYVY, I444 / YUVA and AYUV (an AYUV plane may start at any byte); I420 / I40A / NV12 go
 * through lvk_hip_remap_map_yuv420; every other format is LVK_HIP_ERR_ARG.
 * lvk_hip_lens_apply_obs: the filter, planes in (d_planes / steps as for lvk_hip_ingest_obs), planes of the same format out.  Byte for byte
 *     lvk_hip_ingest_obs -> [test mode: lvk_hip_draw_grid, 32 x 32, col::MAGENTA of lvk_hip_obs_frame_format(video_format), thickness 1]
 *     -> [profile selected: lvk_hip_remap_map(yuv = the frame format is LVK_FORMAT_YUV, bg 0 0 0)] -> lvk_hip_egress_obs
 * in the context's remap precision; without a profile ingest -> [grid] -> egress (the chroma of a subsampled format is the resampled chroma, as in the
 * plugin).  Bytes lvk_hip_egress_obs leaves alone stay the caller's: pitch padding, the alpha planes of I40A / I42A / YUVA (no arguments here), and the
 * last quarter of data[0] of RGBA / BGRA / BGRX, whose DirectIngest moves rows * cols * 3 bytes -- reproduced, not endorsed, as above.  The input planes
 * are never written, in test mode either.  Y800 is a one-channel frame: lvk_hip_lens_apply_gray plane to plane, refused in test mode like it.  The
 * packed frame between the steps is a block of the context's pool that returns to it inside the call.  The handle is left as the packed apply of that
 * frame size leaves it, so the call alternates freely with every other lvk_hip_lens_apply*.
 * Both refuse with LVK_HIP_ERR_ARG, nothing written or enqueued: a NULL lens, d_planes, steps, o_planes or o_steps; what lvk_hip_ingest_obs refuses of
 * the input planes; an output plane that is NULL where the format uses it or whose pitch is below its row; odd cols on 4:2:2, odd rows or cols on 4:2:0;
 * rows or cols below 2 with a profile selected; steps[0] != 4 * cols on RGBA / BGRA / BGRX, in or out; a plane too large for the kernels' 32-bit
 * offsets; an input plane (the source, the map) overlapping an output plane, two output planes overlapping; Y800 in test mode; an unknown format; and --
 * the one refusal the chain has that the fused kernel has not -- an AYUV output plane or pitch that is no multiple of 4 while no profile is selected. */
int  lvk_hip_remap_map_obs(lvk_hip_ctx* ctx, int video_format, const void* d_src, int src_step, int rows, int cols,
                           void* const o_planes[3], const int o_steps[3], const void* d_map, int map_step, const uint8_t bg[3]);
int  lvk_hip_lens_apply_obs(lvk_hip_lens* lens, int video_format, const void* const d_planes[3], const int steps[3],
                            void* const o_planes[3], const int o_steps[3], int rows, int cols);

#ifdef __cplusplus
}
#endif

#include "lvk_hip_scaling_420.h"  /* lvk_hip_scale_yuv420 (PART 2); it includes lvk_hip_scaling_obs.h */
#include "lvk_hip_deblock_420.h"  /* lvk_hip_deblock_apply_yuv420 (PART 2); it includes lvk_hip_deblock_obs.h and, through it, lvk_hip_cas_obs.h and lvk_hip_fsr_obs.h */
#include "lvk_hip_deblock_px.h"   /* lvk_hip_deblock_apply_gray / _c4 (PART 2) */
#endif /* LVK_HIP_H */
