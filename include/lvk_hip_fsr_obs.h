/* liblvk_hip: lvk::FSRFilter on the planes of an I420 / NV12 frame and of every video format FrameIngest::Select accepts, in one call.
 *
 * PART 2 of lvk_hip.h (experimental, no ABI promise), kept in a file of its own and included by lvk_hip.h (through lvk_hip_deblock_420.h,
 * lvk_hip_deblock_obs.h and lvk_hip_cas_obs.h, whose filter follows this one in a CompositeFilter chain): a host includes either.  Plain C.
 */
#ifndef LVK_HIP_FSR_OBS_H
#define LVK_HIP_FSR_OBS_H

#include "lvk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lvk::FSRFilter on the planes of an OBS video format -------------------------------------------------------------------------------------------
 * The FSR 1 EASU pass (lvk_hip_fsr_easu) from a region of a rows x cols frame of `video_format` (LVK_VIDEO_FORMAT_*), planes in (d_planes / steps as for
 * lvk_hip_ingest_obs), to planes of the same format at out_rows x out_cols (o_planes / o_steps as for lvk_hip_egress_obs), out of place, in one call
 * (DESIGN.md section 33).  For every format the output planes are byte for byte those of
 *   lvk_hip_ingest_obs(fmt, d_planes, rows x cols)
 *     -> lvk_hip_fsr_easu(frame, format = lvk_hip_obs_frame_format(fmt), region_xywh, out_rows x out_cols)
 *     -> lvk_hip_egress_obs(fmt, o_planes, out_rows x out_cols)
 * without the two packed frames a host would own between them; for Y800, a one-channel frame, the middle step is lvk_hip_fsr_easu_gray.
 * lvk_hip_fsr_yuv420 is the same for I420 (nv12 = 0: planes Y, U, V) and NV12 (nv12 = 1: planes Y and UV; d_v, v_step, o_v and ov_step are not looked
 * at), with lvk_hip_ingest_yuv420 / lvk_hip_egress_yuv420 as the outer steps; lvk_hip_fsr_obs on I420 / I40A / NV12 is that call.
 * Asynchronous on the context's stream.  The input planes are never written.  Bytes lvk_hip_egress_obs leaves alone stay the caller's: pitch padding, the
 * alpha planes of I40A / I42A / YUVA (no arguments here), and the last quarter of data[0] of RGBA / BGRA / BGRX, whose DirectIngest moves
 * rows * cols * 3 bytes viewed as 3-byte pixels of pitch 3 * cols going in and 3 * out_cols coming out -- reproduced, not endorsed, as for
 * lvk_hip_ingest_obs.  AYUV's A is written as 255.  region_xywh is in pixels of the ingested frame and may start at any, also odd, coordinate.  There is
 * no skip logic here: a 1 : 1 EASU of the whole frame is a legal call (lvk_hip_fsr_geometry tells a host when FSRFilter would skip).
 * The arithmetic is lvk_hip_fsr_easu's on a YUV frame: the shader's r, g, b are Y, U, V.  Three consequences a plane-by-plane scaler gets wrong:
 *   The luma plane out depends on the chroma planes in: the direction analysis runs on 0.5 V + (0.5 Y + U).
 *   The chroma the taps read is the ingest's UP-SAMPLED chroma at frame coordinates (4:2:0: 3 : 1 weights in both directions, the closed form of
 *   lvk_hip_ingest_yuv420; 4:2:2: (far + 3 near + 2) >> 2 along the row; the edge sample replicated).  A region at an odd origin therefore reads the
 *   other chroma phase.
 *   The chroma out is the egress's down-sampling of the scaled full-resolution chroma (4:2:0: (sum of the quad + 2) >> 2; 4:2:2: the pair's sum halved,
 *   half to even).
 * Routes (lvk_hip_fsr_obs_path of the region and the output size: 0 = staged, 1 = direct).  I420 / I40A / NV12, I422 / I42A, YUY2 / YVYU / UYVY,
 * I444 / YUVA and AYUV: staged, ONE launch that reads the planes and writes the planes; direct (downscales past about 1.4 x), lvk_hip_ingest_obs into a
 * frame from the context's pool, which goes back to it inside the call, and one launch from that frame into the planes.  BGR3 and RGBA / BGRA / BGRX:
 * the lvk_hip_fsr_easu kernel on their three-byte pixels from plane to plane; Y800: the lvk_hip_fsr_easu_gray kernel.  No route makes an output-sized
 * packed frame and none ends in lvk_hip_egress_obs: an AYUV plane, in or out, may start at any byte and have any pitch.
 * LVK_HIP_ERR_ARG, with no output byte written and nothing enqueued, for: a NULL context, d_planes, steps, region_xywh, o_planes or o_steps; an unknown
 * format; what lvk_hip_ingest_obs refuses of the input planes at rows x cols; an output plane that is NULL where the format uses it or whose pitch is
 * below its row; odd cols or out_cols on 4:2:2 and odd rows, cols, out_rows or out_cols on 4:2:0; steps[0] != 4 * cols or o_steps[0] != 4 * out_cols on
 * RGBA / BGRA / BGRX; an output plane too large for the kernels' 32-bit offsets; a region that is empty or not inside the frame; out_rows or
 * out_cols <= 0; an input plane's bytes overlapping an output plane's, or two output planes overlapping (there is no in-place form). */
int lvk_hip_fsr_yuv420(lvk_hip_ctx* ctx,
                       const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step, int rows, int cols,
                       const int region_xywh[4],
                       void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int out_rows, int out_cols, int nv12);

int lvk_hip_fsr_obs(lvk_hip_ctx* ctx, int video_format,
                    const void* const d_planes[3], const int steps[3], int rows, int cols, const int region_xywh[4],
                    void* const o_planes[3], const int o_steps[3], int out_rows, int out_cols);

/* host only, no device: 0 = staged, 1 = direct, for the plane kernels of these two entries; LVK_HIP_ERR_ARG for a size <= 0 */
int lvk_hip_fsr_obs_path(int rw, int rh, int out_rows, int out_cols);

#ifdef __cplusplus
}
#endif

#endif /* LVK_HIP_FSR_OBS_H */
