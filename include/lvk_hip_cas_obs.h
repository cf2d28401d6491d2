/* liblvk_hip: lvk::CASFilter on the planes of an I420 / NV12 frame and of every video format FrameIngest::Select accepts, in one call.
 *
 * PART 2 of lvk_hip.h (experimental, no ABI promise), kept in a file of its own and included by lvk_hip.h (through lvk_hip_deblock_420.h and
 * lvk_hip_deblock_obs.h, whose filter this one follows in a CompositeFilter chain): a host includes either.  Plain C.
 */
#ifndef LVK_HIP_CAS_OBS_H
#define LVK_HIP_CAS_OBS_H

#include "lvk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lvk::CASFilter on the planes of an OBS video format -------------------------------------------------------------------------------------------
 * The CAS filter (lvk_hip_cas) on the planes of `video_format` (LVK_VIDEO_FORMAT_*), planes in (d_planes / steps as for lvk_hip_ingest_obs) and planes of
 * the same format and size out (o_planes / o_steps as for lvk_hip_egress_obs), out of place, in one call.  For every format the
 * output planes are byte for byte those of
 *   lvk_hip_ingest_obs(fmt, d_planes) -> lvk_hip_cas(frame, format = lvk_hip_obs_frame_format(fmt), sharpness) -> lvk_hip_egress_obs(fmt, o_planes)
 * without the two packed frames a host would own between them; for Y800, a one-channel frame, the middle step is lvk_hip_cas_gray.
 * lvk_hip_cas_yuv420 is the same for I420 (nv12 = 0: planes Y, U, V) and NV12 (nv12 = 1: planes Y and UV; d_v, v_step, o_v and ov_step are not looked
 * at), with lvk_hip_ingest_yuv420 / lvk_hip_egress_yuv420 as the outer steps; lvk_hip_cas_obs on I420 / I40A / NV12 is that call.
 * Asynchronous on the context's stream.  The input planes are never written.  Bytes lvk_hip_egress_obs leaves alone stay the caller's: pitch padding, the
 * alpha planes of I40A / I42A / YUVA (no arguments here), and the last quarter of data[0] of RGBA / BGRA / BGRX, whose DirectIngest moves
 * rows * cols * 3 bytes viewed as 3-byte pixels -- reproduced, not endorsed, as for lvk_hip_ingest_obs.  AYUV's A is written as 255.
 * CAS sharpens every channel on its own, so no packed pixel exists on the way.  Two consequences of the definition:
 *   Two edge rules meet.  The chroma up-sampling of the ingest REPLICATES the edge sample (4:2:0: 3 : 1 weights in both directions, the closed form of
 *   lvk_hip_ingest_yuv420; 4:2:2: (far + 3 near + 2) >> 2 along the row).  A CAS neighbour OUTSIDE THE FRAME reads as 0 in every channel, which is not
 *   the replicated value.
 *   The chroma out is not a function of the chroma in alone at equal resolution: it is the egress's down-sampling of the sharpened, up-sampled chroma
 *   (4:2:0: INTER_AREA 0.5 x 0.5, (sum of the quad + 2) >> 2; 4:2:2: the pair's sum halved, half to even).  The luma plane out is exactly
 *   lvk_hip_cas_gray of the luma plane in, and each plane of I444 / YUVA exactly lvk_hip_cas_gray of that plane.
 * Routes, one launch each, no copy, no allocation: I420 / I40A / NV12 one kernel that reads the planes and writes the planes; I422 / I42A, YUY2 / YVYU /
 * UYVY, I444 / YUVA and AYUV one kernel per plane layout that does the same; BGR3 and RGBA / BGRA / BGRX the lvk_hip_cas kernel on their three-byte
 * pixels from plane to plane; Y800 the lvk_hip_cas_gray kernel.  No route ends in lvk_hip_egress_obs: an AYUV plane, in or out, may start at any byte
 * and have any pitch.
 * LVK_HIP_ERR_ARG, with no output byte written and nothing enqueued, for: a NULL context, d_planes, steps, o_planes or o_steps; an unknown format; what
 * lvk_hip_ingest_obs refuses of the input planes; an output plane that is NULL where the format uses it or whose pitch is below its row; odd cols on
 * 4:2:2 and odd rows or cols on 4:2:0; steps[0] or o_steps[0] != 4 * cols on RGBA / BGRA / BGRX; an output plane too large for the kernels' 32-bit
 * offsets; a sharpness outside [0, 1] or NaN; an input plane's bytes overlapping an output plane's, or two output planes overlapping (there is no
 * in-place form: the filter and the up-sampling read their neighbours). */
int lvk_hip_cas_yuv420(lvk_hip_ctx* ctx,
                       const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step,
                       void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step,
                       int rows, int cols, int nv12, float sharpness);

int lvk_hip_cas_obs(lvk_hip_ctx* ctx, int video_format,
                    const void* const d_planes[3], const int steps[3],
                    void* const o_planes[3], const int o_steps[3],
                    int rows, int cols, float sharpness);

#ifdef __cplusplus
}
#endif

#include "lvk_hip_fsr_obs.h"  /* lvk_hip_fsr_yuv420 / lvk_hip_fsr_obs: the scaler that precedes this filter in a chain, on the same planes (PART 2) */

#endif /* LVK_HIP_CAS_OBS_H */
