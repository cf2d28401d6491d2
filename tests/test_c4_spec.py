"""The premises of the four-channel (BGRA / RGBA) remap, on the CPU.

The reference has no four-channel EASU program (lvk::remap asserts CV_8UC3).  The remap of a frame (c0, c1, c2, a) is DEFINED through the reference's non-YUV
program -- `yuv=False` in tests/np_easu.py::easu_points and in the oracle: the branch whose luma is `p[..., 0]` --: bytes 0 .. 2 are that program on
(c0, c1, c2), byte 3 is its channel 1 on (c0, a, a).  That is a definition only if output channel k of that program depends on input channels 0 and k alone;
these tests pin it for the oracle and for its numpy twin, at a homography, a materialised map and a 3 x 3 mesh, and show that the YUV program fails the same
test.  The last test holds the C ABI: the seven new symbols are exported by the built library and declared by include/lvk_hip.h."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import np_easu, synth

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["lvk_hip_remap_homography_c4", "lvk_hip_remap_mesh_c4", "lvk_hip_remap_map_c4", "lvk_hip_warpmesh_apply_c4", "lvk_hip_warpmesh_apply_lens_c4",
           "lvk_hip_stab_push_c4", "lvk_hip_stab_push_c4_host"]


def _frame(rows, cols):
    """(c0, c1, c2, a): four planes, none constant and none equal to another"""
    rng = np.random.default_rng(rows * 17 + cols)
    if min(rows, cols) < 32:
        return rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    f = np.empty((rows, cols, 4), np.uint8)
    f[..., :3] = synth.textured_frame(rows, cols, seed=5)
    f[..., 3] = synth.textured_frame(rows, cols, seed=23)[..., 1][::-1]
    return f


def _with(c0, c1, c2):
    return np.ascontiguousarray(np.stack([c0, c1, c2], -1))


def _warps(rows, cols):
    """a rotation that leaves the frame at one side, a smooth offset map, a random 3 x 3 mesh"""
    rng = np.random.default_rng(rows + 3 * cols)
    th = 0.35; c, s = np.cos(th), np.sin(th)
    H = np.array([[c, -s, 0.2 * cols], [s, c, -0.25 * rows], [0, 0, 1]], f32)
    yy, xx = np.mgrid[0:rows, 0:cols]
    m = np.stack([0.37 + 0.01 * yy, -0.61 + 0.02 * xx], -1).astype(f32)
    mesh = synth.random_mesh(3, 3, rng, amp=0.05)
    return H, m, mesh


def _runs(oracle, rows, cols, yuv):
    H, m, mesh = _warps(rows, cols)
    mesh_map = oracle.mesh_to_map(mesh, rows, cols)             # the mesh as the offsets WarpMesh::apply hands the kernel (WarpMesh.cpp:190-191)
    return [("oracle homography", lambda f, bg: oracle.remap_homography(f, H, bg=bg, yuv=yuv)),
            ("numpy homography", lambda f, bg: np_easu.remap_homography(f, H, bg, yuv)),
            ("oracle map", lambda f, bg: oracle.remap_map(f, m, bg=bg, yuv=yuv)),
            ("numpy map", lambda f, bg: np_easu.remap_map(f, m, bg, yuv)),
            ("oracle mesh 3x3", lambda f, bg: oracle.remap_mesh(f, mesh, bg=bg, yuv=yuv)),
            ("numpy mesh 3x3", lambda f, bg: np_easu.remap_map(f, mesh_map, bg, yuv))]


@pytest.mark.parametrize("size", [(6, 7), (41, 57)])
def test_output_channel_k_of_the_non_yuv_program_depends_on_input_channels_0_and_k_only(oracle, size):
    rows, cols = size
    f = _frame(rows, cols)
    c0, c1, c2, a = (f[..., k] for k in range(4))
    rnd = np.random.default_rng(9).integers(0, 256, (rows, cols), dtype=np.uint8)
    zero = np.zeros_like(a)
    for name, run in _runs(oracle, rows, cols, False):
        # byte 3: channel 1 of (c0, a, a) = of (c0, a, 0) = of (c0, a, random) -- the kernels run the core on (c0, a, 0)
        alphas = [run(_with(c0, a, third), (9, 40, bg2))[..., 1] for third, bg2 in ((a, 40), (zero, 0), (rnd, 77))]
        assert np.array_equal(alphas[0], alphas[1]) and np.array_equal(alphas[0], alphas[2]), name
        # bytes 0 and 2 of (c0, c1, c2) do not change when channel 1 is replaced
        base = run(_with(c0, c1, c2), (9, 3, 4))
        for other, bg1 in ((a, 3), (zero, 0), (rnd, 200)):
            got = run(_with(c0, other, c2), (9, bg1, 4))
            assert np.array_equal(got[..., 0], base[..., 0]) and np.array_equal(got[..., 2], base[..., 2]), name
        # ... and the test can tell: channel 1 itself follows its input
        assert not np.array_equal(run(_with(c0, rnd, c2), (9, 3, 4))[..., 1], base[..., 1]), name


def test_the_yuv_program_fails_the_same_test(oracle):
    """The other program's luma mixes the three channels (0.5 x + y + 0.5 z): its weights, and with them every output channel, depend on all of them.  The
    definition therefore names the non-YUV program, and there is no four-channel YUV format."""
    rows, cols = 41, 57
    f = _frame(rows, cols)
    c0, c1, c2, a = (f[..., k] for k in range(4))
    rnd = np.random.default_rng(9).integers(0, 256, (rows, cols), dtype=np.uint8)
    for name, run in _runs(oracle, rows, cols, True):
        assert not np.array_equal(run(_with(c0, a, a), (9, 40, 40))[..., 1], run(_with(c0, a, rnd), (9, 40, 40))[..., 1]), name
        assert not np.array_equal(run(_with(c0, c1, c2), (9, 3, 4))[..., 0], run(_with(c0, rnd, c2), (9, 3, 4))[..., 0]), name


def test_the_library_exports_and_the_header_declares_the_four_channel_entries():
    header = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "livevisionkit_amd", "liblvk_hip.so"))
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} is not declared in include/lvk_hip.h"
        assert hasattr(lib, sym), f"{sym} is not exported by liblvk_hip.so"
    from livevisionkit_amd import _native
    assert all(sym in _native._SIG for sym in SYMBOLS)
