/* liblvk_hip: lvk::ScalingFilter on the planes of an I420 / NV12 frame, in one call.
 *
 * PART 2 of lvk_hip.h (experimental, no ABI promise), kept in a file of its own and included by lvk_hip.h: a host includes either.  Plain C.
 */
#ifndef LVK_HIP_SCALING_420_H
#define LVK_HIP_SCALING_420_H

#include "lvk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lvk::ScalingFilter on 4:2:0 planes -------------------------------------------------------------------------------------------------------
 * The scaling filter (Filters/ScalingFilter.cpp:52-59: lvk::upscale, then lvk::sharpen) on the planes of an I420 / NV12 frame, out of place, in one
 * call: the output planes are byte for byte those of
 *   lvk_hip_ingest_yuv420(d_*) -> lvk_hip_upscale(.., dst size, yuv = 1) -> lvk_hip_sharpen(.., sharpness) -> lvk_hip_egress_yuv420(o_*)
 * without the two packed frames a host would own between them.  Equal sizes sharpen only (lvk::upscale copies, Image.cpp:162-166) in one launch
 * that reads and writes the planes; a larger destination runs the ingest, the YUV EASU program and a sharpening kernel that writes the planes, its
 * two packed frames taken from and given back to the context's pool (lvk_hip_malloc) within the call.  All dst_rows x dst_cols luma bytes and
 * dst_rows / 2 x dst_cols / 2 chroma samples are written and no byte of pitch padding is; the chroma is not a copy of the input even at equal
 * sizes but the INTER_AREA 0.5 of the sharpened, bilinearly up-sampled chroma, as in that chain; sharpness 0 still sharpens (exp2(-2)).
 * nv12 != 0: d_u / o_u are the interleaved UV planes and d_v / o_v are ignored.  Asynchronous on the context's stream.
 * LVK_HIP_ERR_ARG, with no output byte written and nothing enqueued, for: a NULL context; a NULL plane that is in use; any of the four sizes odd
 * or below 2; dst_rows < src_rows or dst_cols < src_cols (Image.cpp:157); a pitch smaller than its row (cols for Y and an NV12 UV plane, cols / 2
 * for I420 chroma); a sharpness outside [0, 1], NaN included; an input plane's bytes overlapping an output plane's, or two output planes
 * overlapping (there is no in-place form: the sharpening and the up-sampling read their neighbours). */
int lvk_hip_scale_yuv420(lvk_hip_ctx* ctx,
                         const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step, int src_rows, int src_cols,
                         void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int dst_rows, int dst_cols,
                         int nv12, float sharpness);

#ifdef __cplusplus
}
#endif

#include "lvk_hip_scaling_obs.h"  /* lvk_hip_scale_obs: the same filter on every OBS video format (PART 2) */

#endif /* LVK_HIP_SCALING_420_H */
