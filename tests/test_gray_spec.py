"""The premises of the one-channel (GRAY) remap, on the CPU.

The reference has no one-channel EASU program (lvk::remap asserts CV_8UC3).  The one-channel remap of a frame g is DEFINED as channel 0 of the reference's
non-YUV program -- `yuv=False` in tests/np_easu.py::easu_points and in the oracle: the branch whose luma is `p[..., 0]` -- run on the three-channel frame
(g, c, c).  That is a definition only if channel 0 of that program does not depend on the other two channels; these tests pin it, for the oracle and for its
numpy twin, together with the other thing the stabilizer tests rely on: the oracle's tracking luma of a YUV frame is channel 0, byte for byte."""
import numpy as np
import pytest

from tests import np_easu, synth


def _three(g, fill, rng=None):
    f = np.empty(g.shape + (3,), np.uint8)
    f[..., 0] = g
    f[..., 1:] = rng.integers(0, 256, g.shape + (2,), dtype=np.uint8) if fill == "random" else fill
    return f


def _cases(rows, cols):
    rng = np.random.default_rng(rows * 131 + cols)
    th = 0.35; c, s = np.cos(th), np.sin(th)
    return [np.array([[1, 0, 0.37], [0, 1, -0.61], [0, 0, 1]], np.float32),
            np.array([[c, -s, 0.2 * cols], [s, c, -0.25 * rows], [0, 0, 1]], np.float32),
            synth.random_homography(rows, cols, rng, strength=2.0)]


@pytest.mark.parametrize("size", [(6, 7), (41, 57)])
def test_channel0_of_the_non_yuv_program_ignores_the_other_channels(oracle, size):
    rows, cols = size
    rng = np.random.default_rng(7)
    g = rng.integers(0, 256, (rows, cols), dtype=np.uint8) if rows < 32 else synth.textured_frame(rows, cols, seed=5)[..., 0].copy()
    frames = [_three(g, 0), _three(g, 128), _three(g, "random", rng)]
    for H in _cases(rows, cols):
        outs = [oracle.remap_homography(f, H, bg=(9, 1 + 50 * i, 200 - 60 * i), yuv=False)[..., 0] for i, f in enumerate(frames)]
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
        twins = [np_easu.remap_homography(f, H, (9, 3, 4), False)[..., 0] for f in frames]
        assert np.array_equal(twins[0], twins[1]) and np.array_equal(twins[0], twins[2])
    mesh = synth.random_mesh(5, 4, rng, amp=0.05)
    outs = [oracle.remap_mesh(f, mesh, bg=(77, 0, 0), yuv=False)[..., 0] for f in frames]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_the_yuv_program_is_not_the_one(oracle):
    """The other program's luma mixes the three channels (0.5 x + y + 0.5 z): its channel 0 DOES depend on them, which is why the definition names the
    non-YUV program -- and why the stabilizer's GRAY tests take the oracle stabilizer's correction and run the oracle's non-YUV remap on it."""
    rng = np.random.default_rng(3)
    g = synth.textured_frame(41, 57, seed=5)[..., 0].copy()
    H = _cases(41, 57)[1]
    a = oracle.remap_homography(_three(g, 128), H, yuv=True)[..., 0]
    b = oracle.remap_homography(_three(g, "random", rng), H, yuv=True)[..., 0]
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("size", [(270, 480), (144, 256), (97, 203)])
def test_oracle_tracking_luma_of_a_yuv_frame_is_channel_0(oracle, size):
    """The oracle stabilizer pushed with format YUV tracks channel 0 (lvko_stab_push_fmt: luma_channel 0): its downscale of (g, 128, 128) equals the
    downscale of the plane g itself, so the tracker sees the GRAY stream's own luma."""
    rows, cols = size
    g = synth.textured_frame(rows, cols, seed=11)[..., 0].copy()
    for (dr, dc) in [(270, 480), (135, 240)]:
        assert np.array_equal(oracle.luma_area_resize(_three(g, 128), dr, dc, channel=0), oracle.luma_area_resize(g, dr, dc))
