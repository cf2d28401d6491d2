/* liblvk_hip: lvk::DeblockingFilter on the planes of an I420 / NV12 frame, in one call.
 *
 * PART 2 of lvk_hip.h (experimental, no ABI promise), kept in a file of its own and included by lvk_hip.h: a host includes either.  Plain C.
 */
#ifndef LVK_HIP_DEBLOCK_420_H
#define LVK_HIP_DEBLOCK_420_H

#include "lvk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lvk::DeblockingFilter on 4:2:0 planes ----------------------------------------------------------------------------------------------------
 * The deblocking filter on the planes of an I420 / NV12 frame, out of place, in one call: the output planes are byte for byte those of
 * lvk_hip_ingest_yuv420(d_*) -> lvk_hip_deblock_apply(packed frame, LVK_FORMAT_YUV) -> lvk_hip_egress_yuv420(o_*), without the packed frame.
 * All rows x cols luma bytes and rows / 2 x cols / 2 chroma samples of the output are written and no byte of pitch padding is; chroma outside the
 * filter region is not a copy of the input but the INTER_AREA 0.5 of its bilinear up-sampling, as in that chain.  nv12 != 0: d_u / o_u are the
 * interleaved UV planes and d_v / o_v are ignored.  rows and cols are even.  Afterwards the handle is in the state lvk_hip_deblock_apply on the
 * ingested frame leaves it in (filter_region, get_grid, draw_influence on a packed 8UC3 frame), and it may alternate with the packed entries at
 * changing sizes.  Asynchronous on the context's stream.  LVK_HIP_ERR_ARG, with nothing changed, for: a NULL plane that is in use; odd or
 * non-positive rows / cols; a pitch smaller than its row (cols for Y and an NV12 UV plane, cols / 2 for I420 chroma); an input plane's bytes
 * overlapping an output plane's, or two output planes overlapping (there is no in-place form: the up-sampling reads its neighbours); and what
 * lvk_hip_deblock_apply refuses (filter_size > 255, no whole macroblock, an empty downscale). */
int lvk_hip_deblock_apply_yuv420(lvk_hip_deblock* deb, const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step,
                                 void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step,
                                 int nv12, int rows, int cols, int region_xywh[4]);

#ifdef __cplusplus
}
#endif

#include "lvk_hip_deblock_obs.h"  /* lvk_hip_deblock_apply_obs: the same filter on every OBS video format (PART 2) */

#endif /* LVK_HIP_DEBLOCK_420_H */
