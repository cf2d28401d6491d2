"""The one- and four-channel EASU upscale and RCAS as DESIGN.md section 22 defines them, evaluated with a THREE-channel upscale / sharpen (the oracle's or
the numpy twin's), and the frames the tests of that section share: the helper of tests/test_scaling_px_spec.py, tests/test_scaling_px_gpu.py and
tests/test_scaling_px_facade.py."""
import numpy as np

from tests import synth


def frame(rows, cols):
    """(c0, c1, c2, a): four planes, none constant and none equal to another (as tests/test_c4_spec.py builds them)"""
    rng = np.random.default_rng(rows * 17 + cols)
    if min(rows, cols) < 32:
        return rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    f = np.empty((rows, cols, 4), np.uint8)
    f[..., :3] = synth.textured_frame(rows, cols, seed=5)
    f[..., 3] = synth.textured_frame(rows, cols, seed=23)[..., 1][::-1]
    return f


def saturate_rings(f):
    """blocks of 0 and of 255 in every plane but the last of a four-channel frame: rings whose limiters are 0 x inf (no-op on a frame too small for them)"""
    rows, cols = f.shape[:2]
    colour = f[..., :3] if f.ndim == 3 and f.shape[2] == 4 else f
    if rows > 40:
        colour[5:9, 5:30] = 0; colour[20:24, 40:70] = 255
    elif rows >= 5 and cols >= 9:
        colour[0:3, 0:3] = 0; colour[rows - 3:, cols - 4:] = 255
    return f


def with_(c0, c1, c2):
    return np.ascontiguousarray(np.stack([c0, c1, c2], -1))


def upscale_gray(upscale3, g, size, c=0):
    """channel 0 of the non-YUV three-channel program on (g, c, c)"""
    return np.ascontiguousarray(upscale3(with_(g, np.full_like(g, c), np.full_like(g, c)), size)[..., 0])


def upscale_c4(upscale3, f, size):
    """bytes 0 .. 2: the program on (c0, c1, c2); byte 3: its channel 1 on (c0, a, a)"""
    colour = upscale3(np.ascontiguousarray(f[..., :3]), size)
    alpha = upscale3(with_(f[..., 0], f[..., 3], f[..., 3]), size)[..., 1]
    return np.ascontiguousarray(np.concatenate([colour, alpha[..., None]], -1))


def sharpen_gray(sharpen3, g, sharpness):
    """any channel of the three-channel program on (g, g, g)"""
    return np.ascontiguousarray(sharpen3(with_(g, g, g), sharpness)[..., 0])


def sharpen_c4(sharpen3, f, sharpness):
    """bytes 0 .. 2: the three-channel program on (c0, c1, c2); byte 3: the source pixel's alpha"""
    return np.ascontiguousarray(np.concatenate([sharpen3(np.ascontiguousarray(f[..., :3]), sharpness), f[..., 3:]], -1))
