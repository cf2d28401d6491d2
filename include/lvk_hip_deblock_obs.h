/* liblvk_hip: lvk::DeblockingFilter on the planes of every video format FrameIngest::Select accepts, in one call.
 *
 * PART 2 of lvk_hip.h (experimental, no ABI promise), kept in a file of its own and included by lvk_hip.h (through lvk_hip_deblock_420.h, whose filter it
 * extends): a host includes either.  Plain C.
 */
#ifndef LVK_HIP_DEBLOCK_OBS_H
#define LVK_HIP_DEBLOCK_OBS_H

#include "lvk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lvk::DeblockingFilter on the planes of an OBS video format ------------------------------------------------------------------------------------
 * The deblocking filter on the planes of `video_format` (LVK_VIDEO_FORMAT_*), planes in (d_planes / steps as for lvk_hip_ingest_obs) and planes of the
 * same format and size out (o_planes / o_steps as for lvk_hip_egress_obs), out of place, in one call.  For every format the output
 * planes are byte for byte those of
 *   lvk_hip_ingest_obs(fmt, d_planes) -> lvk_hip_deblock_apply(frame, format = lvk_hip_obs_frame_format(fmt)) -> lvk_hip_egress_obs(fmt, o_planes)
 * without the packed frame a host would own between them; for Y800, a one-channel frame, the middle step is lvk_hip_deblock_apply_gray.  Asynchronous on
 * the context's stream.  Bytes lvk_hip_egress_obs leaves alone stay the caller's: pitch padding, the alpha planes of I40A / I42A / YUVA (no arguments
 * here), and the last quarter of data[0] of RGBA / BGRA / BGRX, whose DirectIngest moves rows * cols * 3 bytes viewed as 3-byte pixels (RGB for RGBA, BGR
 * for the others) -- reproduced, not endorsed, as for lvk_hip_ingest_obs.  The input planes are never written.  Chroma outside the filter region is that
 * chain's value, not a copy of the input, and a 4:2:2 pair or 4:2:0 quad that straddles the region's edge mixes blended and unblended pixels.
 * Afterwards the handle is in the state lvk_hip_deblock_apply on the ingested frame leaves it in (filter_region, get_grid, draw_influence on a packed
 * 8UC3 frame), and it may alternate with lvk_hip_deblock_apply_yuv420 and the packed entries at changing sizes and formats.
 * Routes: I420 / I40A / NV12 are lvk_hip_deblock_apply_yuv420.  I422 / I42A, YUY2 / YVYU / UYVY, I444 / YUVA and AYUV are four kernels that read the
 * planes and write the planes, with no packed frame.  BGR3, RGBA / BGRA / BGRX and Y800 are one copy into the output plane and the packed apply in place
 * on it.  No route ends in lvk_hip_egress_obs: an AYUV plane, in or out, may start at any byte and have any pitch.
 * LVK_HIP_ERR_ARG, with no output byte written, nothing enqueued and the handle's region and maps as they were, for: a NULL handle, d_planes, steps,
 * o_planes or o_steps; an unknown format; what lvk_hip_ingest_obs refuses of the input planes; an output plane that is NULL where the format uses it or
 * whose pitch is below its row; odd cols on 4:2:2 and odd rows or cols on 4:2:0; steps[0] or o_steps[0] != 4 * cols on RGBA / BGRA / BGRX; an output
 * plane too large for the kernels' 32-bit offsets; an input plane's bytes overlapping an output plane's, or two output planes overlapping (there is no
 * in-place form: the up-sampling reads its neighbours); and what lvk_hip_deblock_apply refuses (filter_size > 255, no whole macroblock, an empty
 * downscale).  region_xywh (may be NULL) receives the filter region. */
int lvk_hip_deblock_apply_obs(lvk_hip_deblock* deb, int video_format,
                              const void* const d_planes[3], const int steps[3],
                              void* const o_planes[3], const int o_steps[3],
                              int rows, int cols, int region_xywh[4]);

#ifdef __cplusplus
}
#endif

#include "lvk_hip_cas_obs.h"  /* lvk_hip_cas_yuv420 / lvk_hip_cas_obs: the filter that follows this one in a chain, on the same planes (PART 2) */

#endif /* LVK_HIP_DEBLOCK_OBS_H */
