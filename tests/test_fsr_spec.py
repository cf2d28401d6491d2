"""CPU pins of the FSR specification (tests/np_fsr.py), of the host logic of the C-ABI (lvk_hip_fsr_easu_const, lvk_hip_fsr_geometry,
lvk_hip_fsr_easu_path) and of its surface.

The restatement is held to hand-checked constant bit patterns, to a geometry table with literal answers, to the point-sampling invariant of
declared choice 6, to flat frames, to the deringing clamp, and to a float64 textbook EASU as a bound.  No device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import np_fsr as nf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(v):
    return [int(b) for b in np.asarray(v, dtype=f32).reshape(-1).view(np.uint32)]


def _lib():
    from livevisionkit_amd import _native
    return _native.load()


# ---- host constants -----------------------------------------------------------------------------------------------------------------

# (rw, rh, W, H, ow, oh) -> con0..con3 as float32 bit patterns, checked by hand: 1 / 1920 = 0x3a088889, 1 / 1080 = 0x3a72b9d6 ...
CON_CASES = {
    (1920, 1080, 1920, 1080, 3840, 2160): [0x3f000000, 0x3f000000, 0xbe800000, 0xbe800000,
                                           0x3a088889, 0x3a72b9d6, 0x3a088889, 0xba72b9d6,
                                           0xba088889, 0x3af2b9d6, 0x3a088889, 0x3af2b9d6,
                                           0x00000000, 0x3b72b9d6, 0x00000000, 0x00000000],
    (1280, 720, 1280, 720, 1920, 1080): [0x3f2aaaab, 0x3f2aaaaa, 0xbe2aaaaa, 0xbe2aaaac,      # 720 rcp(1080) < 1280 rcp(1920)
                                         0x3a4ccccd, 0x3ab60b61, 0x3a4ccccd, 0xbab60b61,
                                         0xba4ccccd, 0x3b360b61, 0x3a4ccccd, 0x3b360b61,
                                         0x00000000, 0x3bb60b61, 0x00000000, 0x00000000],
    (3840, 2160, 3840, 2160, 1920, 1080): [0x40000000, 0x40000000, 0x3f000000, 0x3f000000,
                                           0x39888889, 0x39f2b9d6, 0x39888889, 0xb9f2b9d6,
                                           0xb9888889, 0x3a72b9d6, 0x39888889, 0x3a72b9d6,
                                           0x00000000, 0x3af2b9d6, 0x00000000, 0x00000000],
}


def _hand_con(rw, rh, W, H, ow, oh):
    """The same constants with Python's float64 rounded to float32 after each step (1 / x of a small integer is exact in float64 before
    the final rounding, so each step is the correctly rounded float32 operation)."""
    r = lambda v: float(f32(v))                                               # noqa: E731
    rW, rH, rO, rOh = r(1 / W), r(1 / H), r(1 / ow), r(1 / oh)
    return [r(rw * rO), r(rh * rOh), r(r(r(0.5 * rw) * rO) - 0.5), r(r(r(0.5 * rh) * rOh) - 0.5),
            rW, rH, rW, -rH, -rW, 2 * rH, rW, 2 * rH, 0.0, 4 * rH, 0.0, 0.0]


@pytest.mark.parametrize("case", sorted(CON_CASES))
def test_constant_bit_patterns_of_the_specification_and_the_library(case):
    assert _bits(nf.easu_const(*case)) == CON_CASES[case]
    con = (ctypes.c_float * 16)()
    assert _lib().lvk_hip_fsr_easu_const(*case, con) == 0
    assert _bits(list(con)) == CON_CASES[case]


@pytest.mark.parametrize("case", [(1917, 1001, 1999, 1030, 3001, 777), (7, 5, 13, 11, 1, 1), (1, 1, 1, 1, 4096, 3), (1900, 1080, 1920, 1080, 3800, 2160),
                                  (640, 360, 1920, 1080, 1920, 1080), (3, 4097, 5, 4099, 4096, 4096)])
def test_constants_of_non_power_of_two_sizes(case):
    want = _bits(_hand_con(*case))
    assert _bits(nf.easu_const(*case)) == want
    con = (ctypes.c_float * 16)()
    assert _lib().lvk_hip_fsr_easu_const(*case, con) == 0
    assert _bits(list(con)) == want


def test_constants_refuse_bad_sizes():
    con = (ctypes.c_float * 16)()
    for bad in ((0, 1, 1, 1, 1, 1), (1, 1, 1, 1, 1, -2), (1, 1, 0, 1, 1, 1)):
        assert _lib().lvk_hip_fsr_easu_const(*bad, con) != 0
    assert _lib().lvk_hip_fsr_easu_const(1, 1, 1, 1, 1, 1, None) != 0


# ---- output geometry ----------------------------------------------------------------------------------------------------------------

# (rows, cols, out_size (rows, cols) or None, multiplier, aspect, crop ltrb) -> (region xywh, out (rows, cols), skip)
GEOMETRY = [
    ((1083, 1923, None, 0.5, True, (0, 0, 0, 0)), ((0, 0, 1923, 1083), (542, 962), False)),         # half-even: truncation gives 961 x 541
    ((1083, 1923, None, 0.5, False, (0, 0, 0, 0)), ((0, 0, 1923, 1083), (542, 962), False)),
    ((1080, 1920, None, 2.0, True, (0, 0, 0, 0)), ((0, 0, 1920, 1080), (2160, 3840), False)),
    ((1080, 1920, None, 1.0, True, (0, 0, 0, 0)), ((0, 0, 1920, 1080), (1080, 1920), True)),         # same size, whole frame: pass through
    ((1080, 1920, (1080, 1920), 1.0, False, (0, 0, 0, 0)), ((0, 0, 1920, 1080), (1080, 1920), True)),
    ((1080, 1920, None, 1.0, True, (10, 0, 10, 0)), ((10, 0, 1900, 1080), (1080, 1900), False)),      # same size, cropped: scaled
    ((1080, 1920, None, 1.0, False, (10, 0, 10, 0)), ((10, 0, 1900, 1080), (1080, 1920), False)),
    ((1080, 1920, (2160, 3840), 1.0, True, (10, 0, 10, 0)), ((10, 0, 1900, 1080), (2160, 3800), False)),   # the aspect fit of the issue
    ((1080, 1920, (2160, 3840), 1.0, False, (10, 0, 10, 0)), ((10, 0, 1900, 1080), (2160, 3840), False)),
    ((1080, 1920, None, 1.0, True, (960, 0, 960, 0)), ((0, 0, 1920, 1080), (1080, 1920), True)),      # l + r == W: invalid, whole frame
    ((1080, 1920, None, 1.0, True, (959, 0, 960, 0)), ((959, 0, 1, 1080), (1080, 1), False)),
    ((1080, 1920, None, 1.0, True, (0, 1080, 0, 0)), ((0, 0, 1920, 1080), (1080, 1920), True)),       # t + b == H: invalid
    ((1080, 1920, (2160, 3840), 1.0, True, (0, 0, 0, 4096)), ((0, 0, 1920, 1080), (2160, 3840), False)),
    ((2160, 3840, None, 2.0, True, (0, 0, 0, 0)), ((0, 0, 3840, 2160), (4096, 4096), False)),         # the 4096 cap, after the fit
    ((2160, 3840, (5000, 9000), 1.0, False, (0, 0, 0, 0)), ((0, 0, 3840, 2160), (4096, 4096), False)),
    ((720, 1280, (1080, 4096), 1.0, True, (0, 0, 0, 0)), ((0, 0, 1280, 720), (1080, 1920), False)),
    ((720, 1280, (4096, 4096), 1.0, True, (0, 0, 0, 0)), ((0, 0, 1280, 720), (2304, 4096), False)),
    ((1, 1, None, 0.4, True, (0, 0, 0, 0)), ((0, 0, 1, 1), (0, 0), True)),                            # rounds to 0: skip
    ((3, 3, None, 0.5, True, (0, 0, 0, 0)), ((0, 0, 3, 3), (2, 2), False)),                           # 1.5 -> 2 (half to even)
    ((5, 5, None, 0.5, True, (0, 0, 0, 0)), ((0, 0, 5, 5), (2, 2), False)),                           # 2.5 -> 2
    ((1080, 1920, (0, 1920), 1.0, False, (0, 0, 0, 0)), ((0, 0, 1920, 1080), (0, 1920), True)),       # an explicit 0: skip
    ((1080, 1920, (0, 1920), 1.0, True, (0, 0, 0, 0)), ((0, 0, 1920, 1080), (0, 0), True)),
    ((17, 65, (1, 1), 1.0, False, (3, 2, 1, 4)), ((3, 2, 61, 11), (1, 1), False)),
]


@pytest.mark.parametrize("args,want", GEOMETRY)
def test_geometry_table(args, want):
    assert nf.geometry(*args) == want
    from livevisionkit_amd import fsr_geometry
    assert fsr_geometry(*args) == want


def test_geometry_matches_the_restatement_on_random_settings():
    from livevisionkit_amd import fsr_geometry
    rng = np.random.default_rng(4)
    for _ in range(3000):
        rows, cols = (int(v) for v in rng.integers(1, 5000, 2))
        out = None if rng.random() < 0.5 else tuple(int(v) for v in rng.integers(0, 6000, 2))
        m = float(f32(rng.choice([0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0]) if rng.random() < 0.5 else rng.uniform(0.01, 4)))
        crop = tuple(int(v) for v in rng.integers(0, 2500, 4)) if rng.random() < 0.7 else (0, 0, 0, 0)
        aspect = bool(rng.random() < 0.6)
        assert fsr_geometry(rows, cols, out, m, aspect, crop) == nf.geometry(rows, cols, out, m, aspect, crop), (rows, cols, out, m, aspect, crop)


def test_geometry_refuses_bad_arguments():
    lib = _lib()
    region, size, skip = (ctypes.c_int * 4)(), (ctypes.c_int * 2)(), ctypes.c_int()
    ok = (ctypes.c_int * 4)(0, 0, 0, 0)
    assert lib.lvk_hip_fsr_geometry(10, 10, 0, 0, 1.0, 1, ok, region, size, ctypes.byref(skip)) == 0
    for rows, cols, orow, ocol, m, crop in ((0, 10, 0, 0, 1.0, ok), (10, -1, 0, 0, 1.0, ok), (10, 10, -1, 5, 1.0, ok), (10, 10, 0, 0, 0.0, ok),
                                            (10, 10, 0, 0, -1.0, ok), (10, 10, 0, 0, float("nan"), ok), (10, 10, 0, 0, float("inf"), ok),
                                            (10, 10, 0, 0, 1.0, (ctypes.c_int * 4)(-1, 0, 0, 0)), (10, 10, 0, 0, 1.0, (ctypes.c_int * 4)(0, 0, 4097, 0)),
                                            (10, 10, 0, 0, 1.0, None)):
        assert lib.lvk_hip_fsr_geometry(rows, cols, orow, ocol, m, 1, crop, region, size, ctypes.byref(skip)) != 0
    # the multiplier is not looked at when the size is explicit
    assert lib.lvk_hip_fsr_geometry(10, 10, 5, 5, float("nan"), 1, ok, region, size, ctypes.byref(skip)) == 0
    assert lib.lvk_hip_fsr_geometry(10, 10, 0, 0, 1.0, 1, ok, None, size, ctypes.byref(skip)) != 0


# ---- the sampling invariant (declared choice 6) -------------------------------------------------------------------------------------

def _corpus():
    yield (1, 1, (0, 0, 1, 1), 1, 1)
    yield (1, 1, (0, 0, 1, 1), 7, 3)
    yield (17, 65, (0, 0, 65, 17), 1, 1)
    yield (17, 65, (3, 2, 61, 11), 40, 130)
    yield (1080, 1920, (0, 0, 1920, 1080), 2160, 3840)
    yield (2160, 3840, (0, 0, 3840, 2160), 1080, 1920)
    yield (720, 1280, (0, 0, 1280, 720), 2304, 4096)
    yield (1080, 1920, (480, 270, 960, 540), 1080, 1920)
    yield (2160, 4096, (1, 7, 4093, 2150), 4096, 4096)
    yield (4096, 4096, (13, 0, 4083, 4096), 777, 4096)
    yield (1083, 1923, (0, 0, 1923, 1083), 542, 962)
    yield (4096, 4096, (0, 0, 4096, 4096), 1, 1)
    yield (7, 4096, (4095, 0, 1, 7), 5, 4096)


@pytest.mark.parametrize("case", list(_corpus()))
def test_point_samples_sit_at_texel_centres(case):
    """Every u W the point sampler sees is k + 0.5 +- a small error, so the texel floor(u W) does not depend on how the sampler rounds, and
    it is the integer fp + r + d of the kernel (before the clamp to the frame)."""
    rows, cols, region, oh, ow = case
    worst = 0.0
    for scaled, floor_, integer in nf.sample_coords(rows, cols, region, oh, ow):
        frac = scaled.astype(np.float64) - np.floor(scaled.astype(np.float64))
        worst = max(worst, float(np.max(np.abs(frac - 0.5))))
        assert np.array_equal(floor_, integer)
    assert worst < 0.25, worst


# ---- properties of the restatement -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [nf.FMT_BGR, nf.FMT_RGBA, nf.FMT_YUV])
def test_flat_frames_come_back_exact(fmt):
    ch = nf.CHANNELS[fmt]
    for v in (0, 1, 77, 128, 254, 255):
        for rows, cols, region, oh, ow in ((9, 13, (0, 0, 13, 9), 20, 31), (9, 13, (2, 1, 7, 5), 3, 40), (40, 40, (0, 0, 40, 40), 11, 7)):
            out = nf.fsr(np.full((rows, cols, ch), v, np.uint8), fmt, region, oh, ow)
            assert (out[..., :3] == v).all(), (v, np.unique(out))
            if ch == 4:
                assert (out[..., 3] == 255).all()


def _smooth(rows, cols, seed, ch=3):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols] / np.array([rows, cols]).reshape(2, 1, 1)
    chans = [np.sin(x * rng.uniform(2, 9) + y * rng.uniform(2, 9) + rng.uniform(0, 6)) for _ in range(ch)]
    return np.clip(np.rint(127.5 + 120 * np.stack(chans, -1)), 0, 255).astype(np.uint8)


def test_every_output_lies_within_its_four_nearest_texels():
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for region, oh, ow in (((0, 0, 53, 37), 80, 111), ((5, 3, 40, 30), 17, 19), ((0, 0, 53, 37), 37, 53)):
        out = nf.fsr(img, nf.FMT_RGB, region, oh, ow).astype(int)
        pos = nf._positions(37, 53, region, oh, ow)
        fx = pos[0][1].astype(int) + region[0]
        fy = pos[1][1].astype(int) + region[1]
        lo = np.full(out.shape, 255)
        hi = np.zeros(out.shape, int)
        for dy in (0, 1):
            for dx in (0, 1):
                t = img[np.clip(fy + dy, 0, 36)[:, None], np.clip(fx + dx, 0, 52)[None, :]].astype(int)
                lo, hi = np.minimum(lo, t), np.maximum(hi, t)
        assert (out >= lo).all() and (out <= hi).all()


def test_channel_order_of_the_formats():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (21, 23, 3), dtype=np.uint8)
    bgr = nf.fsr(img, nf.FMT_BGR, (0, 0, 23, 21), 30, 41)
    rgb = nf.fsr(img[..., ::-1].copy(), nf.FMT_RGB, (0, 0, 23, 21), 30, 41)
    assert np.array_equal(bgr, rgb[..., ::-1])
    assert np.array_equal(nf.fsr(img, nf.FMT_YUV, (0, 0, 23, 21), 30, 41), nf.fsr(img, nf.FMT_RGB, (0, 0, 23, 21), 30, 41))
    # the luma is not symmetric in r and b under rounding, so which byte the shader calls red is a declared choice
    u = nf.UNIT
    r, g, b = np.meshgrid(u, u, u, indexing="ij")
    assert ((b * f32(0.5) + (r * f32(0.5) + g)) != (r * f32(0.5) + (b * f32(0.5) + g))).any()
    bgra = np.concatenate([img, rng.integers(0, 256, (21, 23, 1), dtype=np.uint8)], -1)
    out = nf.fsr(bgra, nf.FMT_BGRA, (0, 0, 23, 21), 30, 41)
    assert np.array_equal(out[..., :3], bgr) and (out[..., 3] == 255).all()


@pytest.mark.parametrize("content", ["random", "smooth"])
@pytest.mark.parametrize("shape", [(60, 80, 120, 160), (60, 80, 30, 40), (60, 80, 61, 200)])
def test_bounded_by_the_textbook_easu(content, shape):
    rows, cols, oh, ow = shape
    img = np.random.default_rng(5).integers(0, 256, (rows, cols, 3), dtype=np.uint8) if content == "random" else _smooth(rows, cols, 5)
    d = np.abs(nf.fsr(img, nf.FMT_BGR, (0, 0, cols, rows), oh, ow).astype(int) - nf.textbook_easu(img, nf.FMT_BGR, (0, 0, cols, rows), oh, ow))
    bound = (32, 2.0) if content == "random" else (6, 0.2)         # measured: 30 / 1.77 and 5 / 0.16
    assert d.max() <= bound[0] and d.mean() <= bound[1], (d.max(), d.mean())


def test_approximation_is_not_the_textbook_easu():
    img = np.random.default_rng(5).integers(0, 256, (60, 80, 3), dtype=np.uint8)
    assert not np.array_equal(nf.fsr(img, nf.FMT_BGR, (0, 0, 80, 60), 120, 160), nf.textbook_easu(img, nf.FMT_BGR, (0, 0, 80, 60), 120, 160))


def test_kernel_path_choice():
    lib = _lib()
    assert lib.lvk_hip_fsr_easu_path(1920, 1080, 2160, 3840) == 0          # upscale: staged
    assert lib.lvk_hip_fsr_easu_path(960, 540, 1080, 1920) == 0            # a 1080p centre crop to 1080p
    assert lib.lvk_hip_fsr_easu_path(3840, 2160, 1080, 1920) == 1          # 2x downscale: direct
    assert lib.lvk_hip_fsr_easu_path(1, 1, 1, 1) == 0
    assert lib.lvk_hip_fsr_easu_path(0, 1, 1, 1) != 0 and lib.lvk_hip_fsr_easu_path(1, 1, 1, -1) != 0


# ---- the C-ABI surface --------------------------------------------------------------------------------------------------------------

def _header():
    return open(os.path.join(ROOT, "include", "lvk_hip.h")).read()


def test_header_declares_the_fsr_abi():
    text = _header()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    assert ("int  lvk_hip_fsr_easu(lvk_hip_ctx* ctx, const void* d_src, int src_step, int rows, int cols, int format, const int region_xywh[4], "
            "void* d_dst,\n                      int dst_step, int out_rows, int out_cols);") in stable
    assert re.search(r"int\s+lvk_hip_fsr_geometry\(int rows, int cols, int out_rows, int out_cols, float multiplier, int maintain_aspect_ratio, "
                     r"const int crop_ltrb\[4\],\s+int region_xywh\[4\], int out_rows_cols\[2\], int\* skip\);", stable)
    assert "lvk_hip_fsr_easu(" not in experimental and "lvk_hip_fsr_geometry(" not in experimental
    assert "int lvk_hip_fsr_easu_const(int rw, int rh, int W, int H, int ow, int oh, float con[16]);" in experimental
    assert "lvk_hip_fsr_easu_const(" not in stable and "lvk_hip_fsr_easu_path(" not in stable
    assert int(re.search(r"#define LVK_HIP_ABI_VERSION (\d+)", text).group(1)) >= 10


def test_library_reports_abi_10_and_refuses_without_a_context():
    lib = _lib()
    assert lib.lvk_hip_abi_version() >= 10
    assert b"ABI %d" % lib.lvk_hip_abi_version() in lib.lvk_hip_version()
    region = (ctypes.c_int * 4)(0, 0, 1, 1)
    assert lib.lvk_hip_fsr_easu(None, None, 3, 1, 1, 0, region, None, 3, 1, 1) != 0


def test_python_binding_is_exported():
    import livevisionkit_amd as lvk
    assert {"FSRFilter", "fsr_geometry", "easu_const"} <= set(lvk.__all__)
    assert _bits(lvk.easu_const(1920, 1080, 1920, 1080, 3840, 2160)) == CON_CASES[(1920, 1080, 1920, 1080, 3840, 2160)]
