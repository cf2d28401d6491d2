"""Python mirror of the C-ABI context: device buffers are torch uint8 tensors, work runs on a HIP stream."""
import ctypes

import numpy as np

from . import _native


class LvkHipError(RuntimeError):
    pass


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _u8x3(bg):
    a = np.ascontiguousarray(bg, dtype=np.uint8).reshape(3)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _u8x4(bg):
    a = np.ascontiguousarray(bg, dtype=np.uint8).reshape(4)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _planes420_empty(rows, cols, nv12, device):
    """New output planes of a rows x cols 4:2:0 frame: (y, u, v) for I420, (y, uv [rows/2, cols/2, 2]) for NV12."""
    import torch
    y = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    u = torch.empty((rows // 2, cols // 2, 2) if nv12 else (rows // 2, cols // 2), dtype=torch.uint8, device=device)
    return (y, u) if nv12 else (y, u, torch.empty_like(u))


def _planes420_args(planes, nv12):
    """A plane tuple as the C entries take it: [y, y_step, u, u_step, v, v_step]; NV12 has no V plane (NULL, 0)."""
    a = []
    for p in planes[:2 if nv12 else 3]:
        a += [p.data_ptr(), p.stride(0)]
    return a + ([None, 0] if nv12 else [])


TRACK_CHAIN_GUARD = 64        # LVK_TRACK_CHAIN_GUARD: entries in front of and behind the flow kernel's output buffers
TRACK_CHAIN_FILL = 0xA5       # LVK_TRACK_CHAIN_FILL: every output byte no kernel wrote


class TrackChainDesc(ctypes.Structure):
    """lvk_track_chain_desc (include/lvk_hip.h, PART 2)."""
    _fields_ = [("prev", ctypes.POINTER(ctypes.c_float)), ("matched", ctypes.POINTER(ctypes.c_float)), ("status", ctypes.POINTER(ctypes.c_uint8)),
                ("und", ctypes.POINTER(ctypes.c_float)),
                ("d_prev_img", ctypes.c_void_p), ("prev_step", ctypes.c_int), ("d_next_img", ctypes.c_void_p), ("next_step", ctypes.c_int),
                ("rows", ctypes.c_int), ("cols", ctypes.c_int),
                ("win_w", ctypes.c_int), ("win_h", ctypes.c_int), ("max_level", ctypes.c_int), ("max_count", ctypes.c_int),
                ("epsilon", ctypes.c_double), ("min_eig", ctypes.c_double),
                ("lens", ctypes.c_void_p), ("lens_rows", ctypes.c_int), ("lens_cols", ctypes.c_int), ("lens_sx", ctypes.c_double), ("lens_sy", ctypes.c_double),
                ("n_bound", ctypes.c_int), ("count_on_device", ctypes.c_int), ("n_word", ctypes.c_int),
                ("full", ctypes.c_int), ("model_on_device", ctypes.c_int), ("full_word", ctypes.c_int),
                ("separate_compact", ctypes.c_int), ("host_signal", ctypes.c_int),
                ("threshold", ctypes.c_double), ("region_w", ctypes.c_int), ("region_h", ctypes.c_int)]


class TrackChainResult(ctypes.Structure):
    """lvk_track_chain_result (include/lvk_hip.h, PART 2)."""
    _fields_ = [("H", ctypes.c_double * 9), ("rc", ctypes.c_int), ("signalled", ctypes.c_int), ("count_dev", ctypes.c_int), ("count_host", ctypes.c_int),
                ("mask", ctypes.POINTER(ctypes.c_uint8)), ("pairs_dev", ctypes.POINTER(ctypes.c_float)), ("mirror_matched", ctypes.POINTER(ctypes.c_float)),
                ("mirror_status", ctypes.POINTER(ctypes.c_uint8)),
                ("next_pts", ctypes.POINTER(ctypes.c_float)), ("flow_status", ctypes.POINTER(ctypes.c_uint8)), ("flow_und", ctypes.POINTER(ctypes.c_float))]

REMAP_EXACT, REMAP_1LSB = 0, 1          # LVK_REMAP_EXACT / LVK_REMAP_1LSB of include/lvk_hip.h


def _remap_precision(precision):
    """The C-ABI value of a precision given as REMAP_EXACT / REMAP_1LSB or as "exact" / "1lsb"; anything else goes to the library, which refuses it."""
    if isinstance(precision, str):
        return {"exact": REMAP_EXACT, "1lsb": REMAP_1LSB}.get(precision.lower(), -1)
    return int(precision)


class Context:
    """One HIP stream + staging on one GPU (reference analogue: the implicit cv::ocl queue)."""

    def __init__(self, device=0, stream=None):
        import torch
        if not torch.cuda.is_available():
            raise LvkHipError("no GPU visible: the lvk HIP path has no CPU fallback")
        self.lib = _native.load()
        self.device = device
        torch.cuda.set_device(device)
        self._torch_stream = stream if stream is not None else torch.cuda.current_stream(device)
        handle = ctypes.c_void_p()
        # enqueue on torch's stream so kernels are ordered with the tensors' producers/consumers
        rc = self.lib.lvk_hip_ctx_create_on_stream(device, ctypes.c_void_p(self._torch_stream.cuda_stream), ctypes.byref(handle))
        if rc != 0:
            raise LvkHipError(f"lvk_hip_ctx_create failed ({rc}): {self.lib.lvk_hip_last_error(None).decode()}")
        self.handle = handle

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lvk_hip_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise LvkHipError(f"lvk_hip call failed ({rc}): {self.lib.lvk_hip_last_error(self.handle).decode()}")

    def sync(self):
        self._check(self.lib.lvk_hip_sync(self.handle))

    def set_remap_precision(self, precision):
        """REMAP_EXACT (default: bit-identical to the reference's kernels) or REMAP_1LSB (regrouped tap weights: fewer instructions, every byte within 1)
        for the three-channel remaps of this context: remap_homography / _mesh / _map, warpmesh_apply and its lens / 4:2:0 forms.  Stabilizers have
        their own setting; upscale, sharpen (every pixel size) and the one- and four-channel remaps are exact in both."""
        self._check(self.lib.lvk_hip_set_remap_precision(self.handle, _remap_precision(precision)))

    @property
    def remap_precision(self):
        return self.lib.lvk_hip_get_remap_precision(self.handle)

    # ---- a15/a16 -------------------------------------------------------------------------------
    def remap_homography(self, src, H, bg=(255, 0, 255), yuv=True, out=None, dst_size=None, offset=(0, 0)):
        """lvk::remap(src, dst, homography, background, inverted=true); src/out: torch uint8 [rows, cols, 3] on the GPU."""
        import torch
        rows, cols = src.shape[0], src.shape[1]
        drows, dcols = dst_size if dst_size is not None else (rows, cols)
        if out is None:
            out = torch.empty((drows, dcols, 3), dtype=torch.uint8, device=src.device)
        Ha, Hp = _f32(np.asarray(H, dtype=np.float32).reshape(9))
        bga, bgp = _u8x3(bg)
        self._check(self.lib.lvk_hip_remap_homography(
            self.handle, src.data_ptr(), src.stride(0), rows, cols, out.data_ptr(), out.stride(0), drows, dcols,
            offset[0], offset[1], Hp, bgp, 1 if yuv else 0))
        return out

    def remap_mesh(self, src, mesh, bg=(255, 0, 255), yuv=True, out=None):
        """lvk::remap(src, dst, offset_map, background) with the map interpolated in-kernel from `mesh` [mr, mc, 2]."""
        import torch
        rows, cols = src.shape[0], src.shape[1]
        if out is None:
            out = torch.empty((rows, cols, 3), dtype=torch.uint8, device=src.device)
        m = np.ascontiguousarray(mesh, dtype=np.float32)
        ma, mp = _f32(m)
        bga, bgp = _u8x3(bg)
        self._check(self.lib.lvk_hip_remap_mesh(
            self.handle, src.data_ptr(), src.stride(0), rows, cols, out.data_ptr(), out.stride(0),
            mp, m.shape[0], m.shape[1], bgp, 1 if yuv else 0))
        return out

    def warpmesh_apply(self, src, mesh, bg=(255, 0, 255), yuv=True, out=None):
        """WarpMesh::apply(src, dst, background)."""
        import torch
        rows, cols = src.shape[0], src.shape[1]
        if out is None:
            out = torch.empty((rows, cols, 3), dtype=torch.uint8, device=src.device)
        m = np.ascontiguousarray(mesh, dtype=np.float32)
        ma, mp = _f32(m)
        bga, bgp = _u8x3(bg)
        self._check(self.lib.lvk_hip_warpmesh_apply(
            self.handle, src.data_ptr(), src.stride(0), rows, cols, out.data_ptr(), out.stride(0),
            mp, m.shape[0], m.shape[1], bgp, 1 if yuv else 0))
        return out

    # ---- one-channel (GRAY) and four-channel (BGRA / RGBA) frames: what their methods share; sfx = "_gray" / "_c4", the suffix of the C entries ----------
    def _px_out(self, sfx, src, out, shape=None):
        import torch
        if sfx == "_gray" and src.dim() != 2:
            raise ValueError("a one-channel frame is a [rows, cols] uint8 tensor")
        if sfx == "_c4" and (src.dim() != 3 or src.shape[2] != 4):
            raise ValueError("a four-channel frame is a [rows, cols, 4] uint8 tensor")
        return out if out is not None else torch.empty(tuple(shape or src.shape[:2]) + tuple(src.shape[2:]), dtype=torch.uint8, device=src.device)

    def _px_call(self, name, sfx, src, out, bg, mid, tail=(), shape=None):
        """lvk_hip_<name><sfx>(ctx, the src plane, the out plane, *mid, the background, *tail); out: allocated here when None (shape: not src's)."""
        out = self._px_out(sfx, src, out, shape)
        bga, bgp = (None, int(bg)) if sfx == "_gray" else _u8x4(bg)
        self._check(getattr(self.lib, "lvk_hip_" + name + sfx)(self.handle, src.data_ptr(), src.stride(0), src.shape[0], src.shape[1], out.data_ptr(), out.stride(0),
                                                               *mid, bgp, *tail))
        return out

    def _px_homography(self, sfx, src, H, bg, out, dst_size, offset):
        drows, dcols = dst_size if dst_size is not None else tuple(src.shape[:2])
        Ha, Hp = _f32(np.asarray(H, dtype=np.float32).reshape(9))
        return self._px_call("remap_homography", sfx, src, out, bg, (drows, dcols, offset[0], offset[1], Hp), shape=(drows, dcols))

    def _px_mesh(self, name, sfx, src, mesh, bg, out, lens=None):
        ma, mp = _f32(mesh)
        tail = () if lens is None else ((ctypes.c_double * 9)(*[float(v) for v in lens]),)
        return self._px_call(name, sfx, src, out, bg, (mp, ma.shape[0], ma.shape[1]), tail)

    def _px_map(self, sfx, src, offsets, bg, out):
        return self._px_call("remap_map", sfx, src, out, bg, (offsets.data_ptr(), offsets.stride(0) * 4))

    # ---- one-channel (GRAY) frames: channel 0 of the non-YUV EASU program on (g, c, c); src / out: torch uint8 [rows, cols] -------------
    def remap_homography_gray(self, src, H, bg=0, out=None, dst_size=None, offset=(0, 0)):
        """lvk_hip_remap_homography_gray: remap_homography for a one-channel frame, one background byte."""
        return self._px_homography("_gray", src, H, bg, out, dst_size, offset)

    def remap_mesh_gray(self, src, mesh, bg=0, out=None):
        """lvk_hip_remap_mesh_gray: remap_mesh for a one-channel frame."""
        return self._px_mesh("remap_mesh", "_gray", src, mesh, bg, out)

    def remap_map_gray(self, src, offsets, bg=0, out=None):
        """lvk_hip_remap_map_gray: remap_map for a one-channel frame (offsets: torch float32 [rows, cols, 2] on the GPU, pixels)."""
        return self._px_map("_gray", src, offsets, bg, out)

    def warpmesh_apply_gray(self, src, mesh, bg=0, out=None, lens=None):
        """lvk_hip_warpmesh_apply_gray (lens = camera params: lvk_hip_warpmesh_apply_lens_gray): WarpMesh::apply on a one-channel frame."""
        return self._px_mesh("warpmesh_apply" if lens is None else "warpmesh_apply_lens", "_gray", src, mesh, bg, out, lens)

    # ---- four-channel (BGRA / RGBA) frames: the non-YUV EASU program with a fourth channel under the same weights; src / out: torch uint8
    # [rows, cols, 4], 4-byte aligned, pitches multiples of 4; bg: four bytes ------------------------------------------------------------
    def remap_homography_c4(self, src, H, bg=(255, 0, 255, 255), out=None, dst_size=None, offset=(0, 0)):
        """lvk_hip_remap_homography_c4: remap_homography for a four-channel frame, four background bytes."""
        return self._px_homography("_c4", src, H, bg, out, dst_size, offset)

    def remap_mesh_c4(self, src, mesh, bg=(255, 0, 255, 255), out=None):
        """lvk_hip_remap_mesh_c4: remap_mesh for a four-channel frame."""
        return self._px_mesh("remap_mesh", "_c4", src, mesh, bg, out)

    def remap_map_c4(self, src, offsets, bg=(255, 0, 255, 255), out=None):
        """lvk_hip_remap_map_c4: remap_map for a four-channel frame (offsets: torch float32 [rows, cols, 2] on the GPU, pixels)."""
        return self._px_map("_c4", src, offsets, bg, out)

    def warpmesh_apply_c4(self, src, mesh, bg=(255, 0, 255, 255), out=None):
        """lvk_hip_warpmesh_apply_c4: WarpMesh::apply on a four-channel frame."""
        return self._px_mesh("warpmesh_apply", "_c4", src, mesh, bg, out)

    def warpmesh_apply_lens_c4(self, src, mesh, lens, bg=(255, 0, 255, 255), out=None):
        """lvk_hip_warpmesh_apply_lens_c4: the lens pre-warp (camera params) fused into WarpMesh::apply on a four-channel frame."""
        return self._px_mesh("warpmesh_apply_lens", "_c4", src, mesh, bg, out, lens)

    # ---- a3/a4/a7 image ops --------------------------------------------------------------------------
    def luma_area_resize(self, frame, drows, dcols, channel=0, out=None):
        """frame: torch uint8 [rows, cols, pix] (packed) or [rows, cols] (planar), any base and pitch -> [drows, dcols] uint8 (out: written in place,
        any pitch)."""
        import torch
        pix = frame.shape[2] if frame.dim() == 3 else 1
        if out is None:
            out = torch.empty((drows, dcols), dtype=torch.uint8, device=frame.device)
        self._check(self.lib.lvk_hip_luma_area_resize(self.handle, frame.data_ptr(), frame.stride(0), pix, channel,
                                                      frame.shape[0], frame.shape[1], out.data_ptr(), out.stride(0), drows, dcols))
        return out

    def area_resize_path(self, frame, drows, dcols, channel=0):
        """lvk_hip_area_resize_path: the LVK_AREA_PATH_* form luma_area_resize runs for this frame (its base and pitch count) and these sizes."""
        pix = frame.shape[2] if frame.dim() == 3 else 1
        path = self.lib.lvk_hip_area_resize_path(self.handle, frame.data_ptr(), frame.stride(0), pix, channel, frame.shape[0], frame.shape[1], drows, dcols)
        self._check(min(path, 0))
        return path

    def pyr_down(self, img, out=None):
        import torch
        if out is None:
            out = torch.empty(((img.shape[0] + 1) // 2, (img.shape[1] + 1) // 2), dtype=torch.uint8, device=img.device)
        self._check(self.lib.lvk_hip_pyr_down(self.handle, img.data_ptr(), img.stride(0), img.shape[0], img.shape[1],
                                              out.data_ptr(), out.stride(0)))
        return out

    def scharr(self, img, out=None):
        """out: a contiguous int16 [rows, cols, 2] tensor (the derivative image is tightly packed)."""
        import torch
        if out is None:
            out = torch.empty((img.shape[0], img.shape[1], 2), dtype=torch.int16, device=img.device)
        self._check(self.lib.lvk_hip_scharr(self.handle, img.data_ptr(), img.stride(0), img.shape[0], img.shape[1], out.data_ptr()))
        return out

    def build_pyramid(self, img, max_level=3, win=(11, 11)):
        """Returns [(level uint8 [r, c], deriv int16 [r, c, 2]), ...] as the LK tracker sees them."""
        rows, cols = img.shape
        lv = np.zeros(rows * cols * 2, np.uint8); dv = np.zeros(rows * cols * 4, np.int16)
        lr = np.zeros(8, np.int32); lc = np.zeros(8, np.int32)
        n = self.lib.lvk_hip_build_pyramid(self.handle, img.data_ptr(), img.stride(0), rows, cols, max_level, win[0], win[1],
                                           lv.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), dv.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                                           lr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), lc.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        self._check(min(n, 0))
        out, lo, do = [], 0, 0
        for i in range(n):
            r, c = int(lr[i]), int(lc[i])
            out.append((lv[lo:lo + r * c].reshape(r, c).copy(), dv[do:do + r * c * 2].reshape(r, c, 2).copy()))
            lo += r * c; do += r * c * 2
        return out

    # ---- a5 / a7 ----------------------------------------------------------------------------------------
    def fast_detect(self, img, regions, cap=None):
        """regions: list of (x, y, w, h, threshold, active). Returns a list of [n, 3] int32 (x, y, score) arrays, region-local."""
        rg = np.ascontiguousarray(regions, dtype=np.int32).reshape(-1, 6)
        n = rg.shape[0]
        cap = cap or int(max(1, (rg[:, 2] * rg[:, 3]).max()))
        out = np.zeros((n, cap), np.uint32)
        counts = np.zeros(n, np.int32)
        self._check(self.lib.lvk_hip_fast_detect(self.handle, img.data_ptr(), img.stride(0), img.shape[0], img.shape[1],
                                                 rg.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n,
                                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap,
                                                 counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        res = []
        for i in range(n):
            e = out[i, :min(cap, counts[i])]
            res.append(np.stack([e & 0xFFF, (e >> 12) & 0xFFF, e >> 24], axis=1).astype(np.int32))
        return res, counts

    def pyrlk(self, prev, nxt, pts, win=(11, 11), max_level=3, max_count=5, epsilon=0.01, min_eig=1e-4):
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        out = np.zeros_like(pts)
        st = np.zeros(len(pts), np.uint8)
        self._check(self.lib.lvk_hip_pyrlk(self.handle, prev.data_ptr(), prev.stride(0), nxt.data_ptr(), nxt.stride(0),
                                           prev.shape[0], prev.shape[1],
                                           pts.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(pts),
                                           out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                           st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                           win[0], win[1], max_level, max_count, float(epsilon), float(min_eig)))
        return out, st

    def estimate_global_motion(self, p1, p2, threshold, region=(480, 270), full_homography=True):
        """cv::findHomography(UsacParams) / cv::estimateAffinePartial2D stand-in; returns (n_inliers, H 3x3 float64, mask)."""
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2); p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        H = np.zeros(9, np.float64); mask = np.zeros(len(p1), np.uint8)
        rc = self.lib.lvk_hip_estimate_global_motion(self.handle, p1.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                     p2.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(p1), float(threshold),
                                                     float(region[0]), float(region[1]), 1 if full_homography else 0,
                                                     H.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                     mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        if rc in (-1, -2, -3):
            self._check(rc)
        return rc, H.reshape(3, 3), mask

    def estimate_global_motion_lo(self, p1, p2, threshold, lo_mode, region=(480, 270), full_homography=True):
        """estimate_global_motion with the local optimisation's mode chosen (0: stop at a mask fixed point, the product; 1: every round of the
        specification's loop); returns (n_inliers, H, mask, refit rounds run, left at a fixed point)."""
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2); p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        H = np.zeros(9, np.float64); mask = np.zeros(len(p1), np.uint8); info = (ctypes.c_int * 2)(-1, -1)
        rc = self.lib.lvk_hip_estimate_global_motion_lo(self.handle, p1.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                        p2.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(p1), float(threshold),
                                                        float(region[0]), float(region[1]), 1 if full_homography else 0, int(lo_mode),
                                                        H.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                        mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), info)
        if rc in (-1, -2, -3):
            self._check(rc)
        return rc, H.reshape(3, 3), mask, info[0], info[1]

    # ---- YUV420 <-> packed 444 ----------------------------------------------------------
    def ingest_yuv420(self, y, u, v=None, out=None):
        """I420 (y, u, v) or NV12 (y, uv[r/2, c/2, 2]) torch uint8 planes -> packed [rows, cols, 3]."""
        import torch
        rows, cols = y.shape
        if out is None:
            out = torch.empty((rows, cols, 3), dtype=torch.uint8, device=y.device)
        nv12 = v is None
        self._check(self.lib.lvk_hip_ingest_yuv420(self.handle, *_planes420_args((y, u, v), nv12), 1 if nv12 else 0, rows, cols, out.data_ptr(), out.stride(0)))
        return out

    def egress_yuv420(self, frame, nv12=False, out=None):
        rows, cols = frame.shape[:2]
        if out is None:
            out = _planes420_empty(rows, cols, nv12, frame.device)
        y, u, v = out if not nv12 else (out[0], out[1], None)
        self._check(self.lib.lvk_hip_egress_yuv420(self.handle, frame.data_ptr(), frame.stride(0), rows, cols, *_planes420_args((y, u, v), nv12), 1 if nv12 else 0))
        return (y, u) if nv12 else (y, u, v)

    # ---- every OBS video format of FrameIngest::Select (Modules/OBS-Plugin/Interop/FrameIngest.cpp:36-75) ----------------------
    VIDEO_FORMATS = {"I420": 1, "NV12": 2, "YVYU": 3, "YUY2": 4, "UYVY": 5, "RGBA": 6, "BGRA": 7, "BGRX": 8, "Y800": 9, "I444": 10, "BGR3": 11,
                     "I422": 12, "I40A": 13, "I42A": 14, "YUVA": 15, "AYUV": 16}

    def _obs_args(self, planes):
        import ctypes as c
        ptrs = (c.c_void_p * 3)(*[p.data_ptr() for p in planes] + [None] * (3 - len(planes)))
        steps = (c.c_int * 3)(*[p.stride(0) for p in planes] + [0] * (3 - len(planes)))
        return ptrs, steps

    def ingest_obs(self, fmt, planes, out=None):
        """FrameIngest::to_ocl: the planes OBS holds for one frame of `fmt` (torch uint8, on the GPU) -> the packed frame [rows, cols, 3] ([rows, cols] for Y800)."""
        import torch
        rows, cols = planes[0].shape[:2]
        if out is None:
            out = torch.empty((rows, cols) if fmt == "Y800" else (rows, cols, 3), dtype=torch.uint8, device=planes[0].device)
        ptrs, steps = self._obs_args(planes)
        self._check(self.lib.lvk_hip_ingest_obs(self.handle, self.VIDEO_FORMATS[fmt], ptrs, steps, rows, cols, out.data_ptr(), out.stride(0)))
        return out

    def egress_obs(self, fmt, frame, planes):
        """FrameIngest::to_obs: the frame into the given OBS planes (bytes the reference leaves alone stay what they are)."""
        rows, cols = frame.shape[:2]
        ptrs, steps = self._obs_args(planes)
        self._check(self.lib.lvk_hip_egress_obs(self.handle, self.VIDEO_FORMATS[fmt], frame.data_ptr(), frame.stride(0), rows, cols, ptrs, steps))
        return planes

    def obs_frame_format(self, fmt):
        return self.lib.lvk_hip_obs_frame_format(self.VIDEO_FORMATS[fmt] if isinstance(fmt, str) else int(fmt))

    # ---- lens correction --------------------------------------------------------------------
    def remap_map(self, src, offsets, bg=(255, 0, 255), yuv=True, out=None):
        """lvk::remap(src, dst, offset_map): offsets = torch float32 [rows, cols, 2] on the GPU (pixels)."""
        import torch
        rows, cols = src.shape[:2]
        if out is None:
            out = torch.empty_like(src)
        bga, bgp = _u8x3(bg)
        self._check(self.lib.lvk_hip_remap_map(self.handle, src.data_ptr(), src.stride(0), rows, cols, out.data_ptr(), out.stride(0),
                                               offsets.data_ptr(), offsets.stride(0) * 4, bgp, 1 if yuv else 0))
        return out

    def remap_map_yuv420(self, src, offsets, bg=(255, 0, 255), nv12=False, out=None):
        """lvk_hip_remap_map_yuv420: remap_map(yuv=True) + 4:2:0 egress in one kernel: packed YUV [rows, cols, 3] and offsets [rows, cols, 2] -> (y, u, v)
        I420 or (y, uv) NV12 planes (`out`: the planes to write; allocated when None)."""
        rows, cols = src.shape[0], src.shape[1]
        out = _planes420_empty(rows, cols, nv12, src.device) if out is None else tuple(out)
        bga, bgp = _u8x3(bg)
        self._check(self.lib.lvk_hip_remap_map_yuv420(self.handle, src.data_ptr(), src.stride(0), rows, cols, *_planes420_args(out, nv12), 1 if nv12 else 0,
                                                      offsets.data_ptr(), offsets.stride(0) * 4, bgp))
        return out

    def video_format(self, fmt):
        """The LVK_VIDEO_FORMAT_* number of `fmt`, a name of VIDEO_FORMATS or the number itself."""
        return self.VIDEO_FORMATS[fmt] if isinstance(fmt, str) else int(fmt)

    def remap_map_obs(self, fmt, src, offset_map, planes, bg=(0, 0, 0)):
        """lvk_hip_remap_map_obs: remap_map(yuv=True) + egress_obs(fmt) in one kernel: packed YUV [rows, cols, 3] and offsets [rows, cols, 2] into the
        given planes of `fmt` (a name or a number; I422 / I42A, YUY2 / YVYU / UYVY, I444 / YUVA, AYUV, and I420 / I40A / NV12).  Returns `planes`."""
        rows, cols = src.shape[0], src.shape[1]
        ptrs, steps = self._obs_args(planes)
        bga, bgp = _u8x3(bg)
        self._check(self.lib.lvk_hip_remap_map_obs(self.handle, self.video_format(fmt), src.data_ptr(), src.stride(0), rows, cols, ptrs, steps,
                                                   offset_map.data_ptr(), offset_map.stride(0) * 4, bgp))
        return planes

    def upscale(self, src, size, yuv=True, out=None):
        """lvk::upscale(src, dst, size, yuv): EASU upsampling to size = (width, height) >= the source size."""
        import torch
        rows, cols = src.shape[:2]
        if out is None:
            out = torch.empty((int(size[1]), int(size[0]), 3), dtype=torch.uint8, device=src.device)
        self._check(self.lib.lvk_hip_upscale(self.handle, src.data_ptr(), src.stride(0), rows, cols,
                                             out.data_ptr(), out.stride(0), out.shape[0], out.shape[1], 1 if yuv else 0))
        return out

    def sharpen(self, src, sharpness=0.7, out=None):
        """lvk::sharpen(src, dst, sharpness): RCAS, out of place."""
        import torch
        rows, cols = src.shape[:2]
        if out is None:
            out = torch.empty_like(src)
        self._check(self.lib.lvk_hip_sharpen(self.handle, src.data_ptr(), src.stride(0), rows, cols, out.data_ptr(), out.stride(0),
                                             float(sharpness)))
        return out

    def scale_yuv420(self, y, u, v=None, size=None, sharpness=0.8, out=None):
        """lvk_hip_scale_yuv420: lvk::ScalingFilter on I420 (y, u, v) or NV12 (y, uv[r/2, c/2, 2]; v=None) planes in one call, out of place: the planes of
        ingest_yuv420 -> upscale(size, yuv=True) -> sharpen(sharpness) -> egress_yuv420.  size = (width, height), even and >= the input's; None: the
        input's (sharpen only).  out: the output planes, (y, u, v) or (y, uv).  Returns them."""
        rows, cols = y.shape
        w, h = (cols, rows) if size is None else (int(size[0]), int(size[1]))
        nv12 = v is None
        out = _planes420_empty(h, w, nv12, y.device) if out is None else tuple(out)
        self._check(self.lib.lvk_hip_scale_yuv420(self.handle, *_planes420_args((y, u, v), nv12), rows, cols, *_planes420_args(out, nv12),
                                                  h, w, 1 if nv12 else 0, float(sharpness)))
        return out

    def scale_obs(self, fmt, planes, size=None, sharpness=0.8, out=None):
        """lvk_hip_scale_obs: lvk::ScalingFilter on the planes of one frame of ANY OBS video format in one call, out of place: the planes of
        ingest_obs -> upscale(size, yuv = the frame format is YUV) -> sharpen(sharpness) -> egress_obs (Y800: upscale_gray -> sharpen_gray).  `fmt` = a name
        of VIDEO_FORMATS or its number; `planes` as ingest_obs takes them; size = (width, height) >= the input's, with the format's parity; None: the
        input's (sharpen only).  `out` = the planes of the output frame (allocated when None -- every plane of a format has the frame's size or half of
        it, so plane i is the input's plane i at the new size; bytes the egress leaves alone are then undefined).  Returns `out`."""
        import torch
        planes = list(planes)
        rows, cols = int(planes[0].shape[0]), int(planes[0].shape[1])
        w, h = (cols, rows) if size is None else (int(size[0]), int(size[1]))
        if out is None:
            out = [torch.empty((p.shape[0] * h // rows, p.shape[1] * w // cols, *p.shape[2:]), dtype=torch.uint8, device=p.device) for p in planes]
        else:
            out = list(out)
        if len(out) != len(planes):
            raise ValueError("`out` holds one plane per input plane")
        iptr, istep = self._obs_args(planes)
        optr, ostep = self._obs_args(out)
        self._check(self.lib.lvk_hip_scale_obs(self.handle, self.video_format(fmt), iptr, istep, rows, cols, optr, ostep, h, w, float(sharpness)))
        return out

    # ---- ScalingFilter's two steps on one-channel ([rows, cols]) and four-channel ([rows, cols, 4]; 4-byte aligned, pitches multiples of 4) frames ----
    def _px_upscale(self, sfx, src, size, out):
        out = self._px_out(sfx, src, out, (int(size[1]), int(size[0])))
        self._check(getattr(self.lib, "lvk_hip_upscale" + sfx)(self.handle, src.data_ptr(), src.stride(0), src.shape[0], src.shape[1],
                                                               out.data_ptr(), out.stride(0), out.shape[0], out.shape[1]))
        return out

    def _px_sharpen(self, sfx, src, sharpness, out):
        out = self._px_out(sfx, src, out)
        self._check(getattr(self.lib, "lvk_hip_sharpen" + sfx)(self.handle, src.data_ptr(), src.stride(0), src.shape[0], src.shape[1],
                                                               out.data_ptr(), out.stride(0), float(sharpness)))
        return out

    def upscale_gray(self, src, size, out=None):
        """lvk_hip_upscale_gray: EASU upsampling of a one-channel frame to size = (width, height): channel 0 of upscale(yuv=False) on (g, c, c)."""
        return self._px_upscale("_gray", src, size, out)

    def upscale_c4(self, src, size, out=None):
        """lvk_hip_upscale_c4: EASU upsampling of a four-channel frame; the alpha is resampled under the colour's weights."""
        return self._px_upscale("_c4", src, size, out)

    def sharpen_gray(self, src, sharpness=0.7, out=None):
        """lvk_hip_sharpen_gray: RCAS of a one-channel frame, out of place: any channel of sharpen on (g, g, g)."""
        return self._px_sharpen("_gray", src, sharpness, out)

    def sharpen_c4(self, src, sharpness=0.7, out=None):
        """lvk_hip_sharpen_c4: RCAS of the three colour bytes of a four-channel frame, out of place; the alpha byte is the source pixel's."""
        return self._px_sharpen("_c4", src, sharpness, out)

    def mesh_solver(self, cols, rows, gen_region=(480, 270), temporal=1.0, local=20.0, max_points=4096):
        """FrameTracker's local-motion solver (stage a10) as an object with .solve(tracked, matched, ...), .reset(), .close()."""
        return MeshSolver(self, cols, rows, gen_region, temporal, local, max_points)

    def native_rcp(self, x):
        """native_recip of FSR.cl as this device defines it (v_rcp_f32), elementwise; x: torch float32 on the GPU."""
        import torch
        x = x.contiguous()
        out = torch.empty_like(x)
        self._check(self.lib.lvk_hip_native_rcp(self.handle, x.data_ptr(), out.data_ptr(), x.numel()))
        return out

    def lens_map(self, params, rows, cols):
        """Device offset map of LCFilter for camera params (fx, fy, cx, cy, k1, k2, p1, p2, k3): (torch view [rows, cols, 2], view_xywh)."""
        import torch
        arr = (ctypes.c_double * 9)(*[float(v) for v in params])
        d = ctypes.c_void_p(); view = (ctypes.c_int * 4)()
        self._check(self.lib.lvk_hip_lens_map_create(self.handle, arr, rows, cols, ctypes.byref(d), view))
        # hand ownership to torch: stage through host once (the map is static per profile / frame size)
        tmp = np.zeros((rows, cols, 2), np.float32)
        self._check(self.lib.lvk_hip_download(self.handle, tmp.ctypes.data_as(ctypes.c_void_p), d, tmp.nbytes))
        self.sync()
        t = torch.from_numpy(tmp).to("cuda")
        self._check(self.lib.lvk_hip_lens_map_destroy(self.handle, d))
        return t, tuple(view)

    def warpmesh_apply_lens(self, src, mesh, params, bg=(255, 0, 255), yuv=True, out=None):
        """WarpMesh::apply on the lens-corrected frame, sampled from the RAW frame `src` in one pass (fused lens mode)."""
        import torch
        rows, cols = src.shape[0], src.shape[1]
        if out is None:
            out = torch.empty((rows, cols, 3), dtype=torch.uint8, device=src.device)
        m = np.ascontiguousarray(mesh, dtype=np.float32)
        ma, mp = _f32(m)
        bga, bgp = _u8x3(bg)
        arr = (ctypes.c_double * 9)(*[float(v) for v in params])
        self._check(self.lib.lvk_hip_warpmesh_apply_lens(self.handle, src.data_ptr(), src.stride(0), rows, cols, out.data_ptr(), out.stride(0),
                                                         mp, m.shape[0], m.shape[1], bgp, 1 if yuv else 0, arr))
        return out

    def lens_undistort_points(self, params, rows, cols, sx, sy, pts):
        """Raw tracking-frame points -> lens-corrected positions (binary64 on the GPU)."""
        p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        out = np.zeros_like(p)
        arr = (ctypes.c_double * 9)(*[float(v) for v in params])
        fp = ctypes.POINTER(ctypes.c_float)
        self._check(self.lib.lvk_hip_lens_undistort_points(self.handle, arr, rows, cols, float(sx), float(sy), p.ctypes.data_as(fp), len(p), out.ctypes.data_as(fp)))
        return out

    # ---- debug overlays ---------------------------------------------------------------------
    def draw_grid(self, frame, grid, colour, thickness=1):
        """lvk::draw_grid(dst, grid = (w, h) cells, colour, thickness): draws into `frame` in place."""
        ca, cp = _u8x3(colour)
        self._check(self.lib.lvk_hip_draw_grid(self.handle, frame.data_ptr(), frame.stride(0), frame.shape[0], frame.shape[1], int(grid[0]), int(grid[1]), cp, thickness))
        return frame

    def draw_crosses(self, frame, points, colour, cross_size, thickness, scaling=(1.0, 1.0)):
        """lvk::draw_crosses(dst, points, colour, size, thickness, coord_scaling): draws into `frame` in place."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        ca, cp = _u8x3(colour)
        self._check(self.lib.lvk_hip_draw_crosses(self.handle, frame.data_ptr(), frame.stride(0), frame.shape[0], frame.shape[1],
                                                  p.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(p), float(scaling[0]), float(scaling[1]), cp,
                                                  int(cross_size), int(thickness)))
        return frame

    def fast_filter(self, prev, matched, status):
        """GPU-side fast_filter of the flow result: (kept prev, kept matched) in the reference's swap-erase order."""
        a = np.ascontiguousarray(prev, np.float32).reshape(-1, 2); b = np.ascontiguousarray(matched, np.float32).reshape(-1, 2)
        st = np.ascontiguousarray(status, np.uint8).reshape(-1)
        oa = np.zeros_like(a); ob = np.zeros_like(b)
        fp = ctypes.POINTER(ctypes.c_float)
        m = self.lib.lvk_hip_fast_filter(self.handle, a.ctypes.data_as(fp), b.ctypes.data_as(fp), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(a),
                                         oa.ctypes.data_as(fp), ob.ctypes.data_as(fp))
        if m < 0:
            self._check(m)
        return oa[:m], ob[:m]

    def track_chain(self, prev, matched=None, status=None, und=None, images=None, win=(11, 11), max_level=3, max_count=5, epsilon=0.01, min_eig=1e-4,
                    lens=None, threshold=3.0, region=(480, 270), full=True, full_word=None, n_word=None, separate_compact=False, host_signal=False):
        """The tracker's chain (optical flow ->) fast_filter -> global motion through the launcher the stabilization filter uses (lvk_hip_track_chain).
        Starts from a flow result (prev, matched, status[, und = corrected (previous | matched) positions]) or from images = (prev, next) device
        tensors; lens = (params, frame_rows, frame_cols, sx, sy).  n_word / full_word: the count / the model choice travel in device memory
        (len(prev) is then the launch bound, `full` a placeholder the word overrides).  Returns a dict of everything the entry reports."""
        fp, bp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8)
        prev = np.ascontiguousarray(prev, np.float32).reshape(-1, 2)
        nb, G = len(prev), TRACK_CHAIN_GUARD
        d, r = TrackChainDesc(), TrackChainResult()
        keep = [prev]
        d.prev = prev.ctypes.data_as(fp)
        if images is None:
            matched = np.ascontiguousarray(matched, np.float32).reshape(nb, 2); status = np.ascontiguousarray(status, np.uint8).reshape(nb)
            keep += [matched, status]
            d.matched = matched.ctypes.data_as(fp); d.status = status.ctypes.data_as(bp)
            if und is not None:
                und = np.ascontiguousarray(und, np.float32).reshape(-1, 2)
                n_eff = nb if n_word is None else min(max(int(n_word), 0), nb)
                if len(und) != 2 * n_eff:
                    raise ValueError("und holds 2 x the effective count of positions (previous | matched)")
                keep.append(und)
                d.und = und.ctypes.data_as(fp)
        else:
            a, b = images
            keep += [a, b]
            d.d_prev_img = a.data_ptr(); d.prev_step = a.stride(0); d.d_next_img = b.data_ptr(); d.next_step = b.stride(0)
            d.rows, d.cols = a.shape[0], a.shape[1]
            d.win_w, d.win_h, d.max_level, d.max_count, d.epsilon, d.min_eig = win[0], win[1], max_level, max_count, float(epsilon), float(min_eig)
            if lens is not None:
                params, lrows, lcols, sx, sy = lens
                arr = (ctypes.c_double * 9)(*[float(v) for v in params])
                keep.append(arr)
                d.lens = ctypes.cast(arr, ctypes.c_void_p); d.lens_rows, d.lens_cols, d.lens_sx, d.lens_sy = int(lrows), int(lcols), float(sx), float(sy)
        d.n_bound = nb
        d.count_on_device, d.n_word = (0, 0) if n_word is None else (1, int(n_word))
        d.full = 1 if full else 0
        d.model_on_device, d.full_word = (0, 0) if full_word is None else (1, int(full_word))
        d.separate_compact = 1 if separate_compact else 0; d.host_signal = 1 if host_signal else 0
        d.threshold = float(threshold); d.region_w, d.region_h = int(region[0]), int(region[1])
        mask = np.zeros(nb, np.uint8); pairs = np.zeros((2, nb, 2), np.float32); mm = np.zeros((nb, 2), np.float32); ms = np.zeros(nb, np.uint8)
        r.mask = mask.ctypes.data_as(bp); r.pairs_dev = pairs.ctypes.data_as(fp); r.mirror_matched = mm.ctypes.data_as(fp); r.mirror_status = ms.ctypes.data_as(bp)
        out = {}
        if images is not None:
            nxt = np.zeros((nb + 2 * G, 2), np.float32); fst = np.zeros(nb + 2 * G, np.uint8); fund = np.zeros((2 * nb + 2 * G, 2), np.float32)
            r.next_pts = nxt.ctypes.data_as(fp); r.flow_status = fst.ctypes.data_as(bp); r.flow_und = fund.ctypes.data_as(fp)
            out.update(next_pts=nxt, flow_status=fst, flow_und=fund)
        self._check(self.lib.lvk_hip_track_chain(self.handle, ctypes.byref(d), ctypes.byref(r)))
        del keep
        out.update(H=np.array(r.H, np.float64).reshape(3, 3), rc=r.rc, signalled=r.signalled, count_dev=r.count_dev, count_host=r.count_host, mask=mask,
                   pairs_dev=pairs, mirror_matched=mm, mirror_status=ms)
        return out

    def warpmesh_apply_yuv420(self, src, mesh, bg=(255, 0, 255), nv12=False):
        """WarpMesh::apply + 4:2:0 egress in one kernel: packed YUV [rows, cols, 3] -> (y, u, v) I420 or (y, uv) NV12 planes."""
        rows, cols = src.shape[0], src.shape[1]
        out = _planes420_empty(rows, cols, nv12, src.device)
        m = np.ascontiguousarray(mesh, dtype=np.float32)
        ma, mp = _f32(m)
        bga, bgp = _u8x3(bg)
        self._check(self.lib.lvk_hip_warpmesh_apply_yuv420(self.handle, src.data_ptr(), src.stride(0), rows, cols, *_planes420_args(out, nv12), 1 if nv12 else 0,
                                                           mp, m.shape[0], m.shape[1], bgp))
        return out


class MeshSolver:
    """lvk_hip_mesh_solver_*: FrameTracker::estimate_local_motions on the device; keeps the previous solution between calls."""

    def __init__(self, ctx, cols, rows, gen_region, temporal, local, max_points):
        self.ctx, self.cols, self.rows = ctx, cols, rows
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.lvk_hip_mesh_solver_create(ctx.handle, cols, rows, float(gen_region[0]), float(gen_region[1]), float(temporal), float(local),
                                                      int(max_points), ctypes.byref(h)))
        self.handle = h

    def solve(self, tracked, matched, region=(480, 270), temporal=1.0, threshold=10.0):
        """Returns (status, inliers uint8 [n], offsets float32 [rows, cols, 2]); status 0 = estimate, 2 / 3 = none."""
        t = np.ascontiguousarray(tracked, np.float32).reshape(-1, 2); m = np.ascontiguousarray(matched, np.float32).reshape(-1, 2)
        inl = np.zeros(len(t), np.uint8); off = np.zeros((self.rows, self.cols, 2), np.float32)
        fp = ctypes.POINTER(ctypes.c_float)
        rc = self.ctx.lib.lvk_hip_mesh_solver_solve(self.handle, t.ctypes.data_as(fp), m.ctypes.data_as(fp), len(t), float(region[0]), float(region[1]),
                                                    float(temporal), float(threshold), inl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), off.ctypes.data_as(fp))
        if rc < 0:
            self.ctx._check(rc)
        return rc, inl, off

    def reset(self):
        self.ctx._check(self.ctx.lib.lvk_hip_mesh_solver_reset(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):          # (never hand the library a solver whose context is gone)
                self.ctx.lib.lvk_hip_mesh_solver_destroy(self.handle)
            self.handle = None
