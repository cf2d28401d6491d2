/* liblvk_hip: lvk::DeblockingFilter on one-channel (GRAY) and four-channel (BGRA / RGBA) frames.
 *
 * PART 2 of lvk_hip.h (experimental, no ABI promise), kept in a file of its own and included by lvk_hip.h: a host includes either.  Plain C.
 */
#ifndef LVK_HIP_DEBLOCK_PX_H
#define LVK_HIP_DEBLOCK_PX_H

#include "lvk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lvk::DeblockingFilter on one- and four-channel frames ------------------------------------------------------------------------------------------
 * lvk_hip_deblock_apply of lvk_hip.h (PART 1) for a GRAY frame (8UC1) and for a BGRA / RGBA frame (8UC4), on the same handle: IN PLACE on the region of whole
 * macroblocks, asynchronous on the context's stream, *region_xywh (optional) = that region.  Unlike the one- and four-channel scaling entries of lvk_hip.h these are no definitions of
 * ours: the reference's filter is made of channel-agnostic OpenCV calls (Filters/DeblockingFilter.cpp:48-110: cv::resize, cv::medianBlur, reformatTo(GRAY),
 * cv::blendLinear), and the two entries run them per channel as the three-channel entry does (tests/np_deblock_px.py):
 *   GRAY: the grey image of the block statistics is the frame itself;
 *   four channels: the grey is the fixed-point BT.601 of the colour bytes (BGRA2GRAY / RGBA2GRAY, alpha ignored; `format` tells which byte is blue), and the
 *     ALPHA byte is a channel like the others: downscaled, median-filtered, up-sampled and blended under the same keep map, because that is what those
 *     calls do to an 8UC4 UMat.  This differs on purpose from lvk_hip_sharpen_c4 and the four-channel remaps, where alpha had no reference program.
 * The blend maps are independent of the pixel size: lvk_hip_deblock_draw_influence (8UC3 frames only, as in the reference, whose overlay is an 8UC3
 * buffer), lvk_hip_deblock_filter_region and lvk_hip_deblock_get_grid work after either entry as after lvk_hip_deblock_apply.
 * Refused with LVK_HIP_ERR_ARG, the frame and the filter (region, maps, tap) as they were: a NULL frame, rows or cols <= 0, step < BPP * cols,
 * filter_size > 255, a frame without one whole macroblock or whose 1 / filter_scaling downscale is empty; for `_c4` also a format other than
 * LVK_FORMAT_BGRA / LVK_FORMAT_RGBA and a base or pitch that is not a multiple of 4.  `_gray` takes any base address and any pitch. */
int lvk_hip_deblock_apply_gray(lvk_hip_deblock* deb, void* d_frame, int step, int rows, int cols, int region_xywh[4]);
int lvk_hip_deblock_apply_c4(lvk_hip_deblock* deb, void* d_frame, int step, int rows, int cols, int format, int region_xywh[4]);

#ifdef __cplusplus
}
#endif

#endif /* LVK_HIP_DEBLOCK_PX_H */
