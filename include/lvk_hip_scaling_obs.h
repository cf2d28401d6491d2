/* liblvk_hip: lvk::ScalingFilter on the planes of every video format FrameIngest::Select accepts, in one call.
 *
 * PART 2 of lvk_hip.h (experimental, no ABI promise), kept in a file of its own and included by lvk_hip.h (through lvk_hip_scaling_420.h, whose filter it
 * extends): a host includes either.  Plain C.
 */
#ifndef LVK_HIP_SCALING_OBS_H
#define LVK_HIP_SCALING_OBS_H

#include "lvk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lvk::ScalingFilter on the planes of an OBS video format --------------------------------------------------------------------------------------
 * The scaling filter (Filters/ScalingFilter.cpp:52-59: lvk::upscale, then lvk::sharpen) on the planes of `video_format` (LVK_VIDEO_FORMAT_*), planes in
 * (d_planes / steps as for lvk_hip_ingest_obs, at src_rows x src_cols) and planes of the same format out (o_planes / o_steps as for lvk_hip_egress_obs,
 * at dst_rows x dst_cols), out of place, in one call.  For every format the output planes are byte for byte those of
 *   lvk_hip_ingest_obs(fmt, d_planes, src size) -> lvk_hip_upscale(.., dst size, yuv = (lvk_hip_obs_frame_format(fmt) == LVK_FORMAT_YUV))
 *     -> lvk_hip_sharpen(.., sharpness) -> lvk_hip_egress_obs(fmt, o_planes, dst size)
 * without the three packed frames a host would own between them; for Y800, a one-channel frame, of lvk_hip_upscale_gray -> lvk_hip_sharpen_gray, plane
 * to plane.  Equal sizes sharpen only (lvk::upscale copies, Image.cpp:162-166); sharpness 0 still sharpens (exp2(-2)).  Asynchronous on the context's
 * stream.  Bytes lvk_hip_egress_obs leaves alone stay the caller's: pitch padding, the alpha planes of I40A / I42A / YUVA (no arguments here), and the
 * last quarter of data[0] of RGBA / BGRA / BGRX, whose DirectIngest moves rows * cols * 3 bytes viewed as 3-byte pixels -- reproduced, not endorsed, as
 * for lvk_hip_ingest_obs; the view is taken at the source size going in and at the destination size coming out.  The input planes are never written.
 * Routes: I420 / I40A / NV12 are lvk_hip_scale_yuv420.  I422 / I42A, YUY2 / YVYU / UYVY, I444 / YUVA and AYUV at equal sizes are ONE kernel that reads
 * the planes and writes the planes; at a larger destination the ingest and the YUV EASU program run into two packed frames and a sharpening kernel
 * writes the planes from the second.  BGR3 and RGBA / BGRA / BGRX run lvk_hip_upscale(yuv = 0) and lvk_hip_sharpen on their three-byte pixels, Y800 the
 * two gray kernels.  Every frame between two launches is a block of the context's pool (lvk_hip_malloc) that returns to it inside the call.
 * No route ends in lvk_hip_egress_obs: an AYUV plane, in or out, may start at any byte and have any pitch.
 * LVK_HIP_ERR_ARG, with no output byte written and nothing enqueued, for: a NULL ctx, d_planes, steps, o_planes or o_steps; an unknown format; what
 * lvk_hip_ingest_obs refuses of the input planes at the source size; an output plane that is NULL where the format uses it or whose pitch is below its
 * row at the destination size; odd cols on 4:2:2 and odd rows or cols on 4:2:0, at either size; steps[0] != 4 * src_cols or o_steps[0] != 4 * dst_cols
 * on RGBA / BGRA / BGRX; dst_rows < src_rows or dst_cols < src_cols (Image.cpp:157); a sharpness outside [0, 1], NaN included; a plane too large for
 * the kernels' 32-bit offsets; an input plane's bytes overlapping an output plane's, or two output planes overlapping (there is no in-place form: the
 * sharpening and the up-sampling read their neighbours). */
int lvk_hip_scale_obs(lvk_hip_ctx* ctx, int video_format,
                      const void* const d_planes[3], const int steps[3], int src_rows, int src_cols,
                      void* const o_planes[3], const int o_steps[3], int dst_rows, int dst_cols,
                      float sharpness);

#ifdef __cplusplus
}
#endif

#endif /* LVK_HIP_SCALING_OBS_H */
