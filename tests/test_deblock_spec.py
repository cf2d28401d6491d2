"""CPU pins of the deblocking specification (tests/np_deblock.py) and of its C-ABI surface.

The restatement is held to third-party and frozen implementations where they exist (scipy's median filter, the oracle's INTER_AREA),
to closed forms where they do not, and the header / library are checked for the lvk_hip_deblock_* entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import np_deblock as nd
from tests.deblock_px_cases import CASES, NOT_LIVE, case_id, expected3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(rows, cols, seed, blocky=False):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    if blocky:
        # flat 8 x 8 blocks with a little noise: what a compressed frame looks like to the filter
        base = rng.integers(0, 256, ((rows + 7) // 8, (cols + 7) // 8, 3))
        base = np.repeat(np.repeat(base, 8, axis=0), 8, axis=1)[:rows, :cols]
        f = np.clip(base + rng.integers(-2, 3, (rows, cols, 3)), 0, 255).astype(np.uint8)
    return f


@pytest.mark.parametrize("k", [3, 5, 7, 9])
def test_median_is_scipy_median_filter_nearest(k):
    ndimage = pytest.importorskip("scipy.ndimage")
    img = _frame(37, 53, seed=k)
    got = nd.median(img, k)
    for c in range(3):
        want = ndimage.median_filter(img[..., c], size=k, mode="nearest")
        assert np.array_equal(got[..., c], want), c


@pytest.mark.parametrize("k", [2, 3, 4, 16])
def test_integer_area_steps_equal_the_oracle(oracle, k):
    img = _frame(9 * k, 13 * k, seed=k)
    got = nd.area_resize(img, 9, 13, float(k))
    for c in range(3):
        assert np.array_equal(got[..., c], oracle.luma_area_resize(img, 9, 13, channel=c)), c


@pytest.mark.parametrize("shape,dst", [((100, 150), (40, 60)), ((64, 96), (24, 36)), ((70, 77), (20, 22))])
def test_general_area_tables_equal_the_oracle(oracle, shape, dst):
    # the oracle scales each axis by ssize / dsize; these shapes have one scale for both axes (2.5, 8 / 3, 3.5)
    img = _frame(*shape, seed=5)
    scale = shape[1] / dst[1]
    assert scale == shape[0] / dst[0]
    got = nd.area_resize(img, dst[0], dst[1], scale)
    for c in range(3):
        assert np.array_equal(got[..., c], oracle.luma_area_resize(img, dst[0], dst[1], channel=c)), c


@pytest.mark.parametrize("fmt,channel", [(nd.FMT_BGR, -1), (nd.FMT_RGB, -2), (nd.FMT_YUV, 0)])
def test_gray_block_grid_equals_the_oracle(oracle, fmt, channel):
    img = _frame(48, 80, seed=fmt)
    got = nd.block_grid(nd.gray_of(img, fmt), 16)
    assert np.array_equal(got, oracle.luma_area_resize(img, 3, 5, channel=channel))


def test_small_size_and_scale_of_the_inverse_downscale():
    # saturate_cast<int>(n * (double)(1.f / s)) and scale = 1 / (double)(1.f / s)
    assert nd.small_size(3840, 4.0) == 960 and nd.small_size(1072, 4.0) == 268
    assert nd.small_size(70, 4.0) == 18              # 17.5 rounds to even: the last cell reaches past the region
    assert nd.small_size(66, 4.0) == 16              # 16.5 rounds to even
    scale3 = 1.0 / float(np.float32(1) / np.float32(3))
    assert scale3 != 3.0 and abs(scale3 - 3.0) < 1e-6       # s = 3 runs the general area tables
    assert 1.0 / float(np.float32(1) / np.float32(4)) == 4.0


def test_partial_cells_average_what_they_cover():
    img = np.full((6, 10, 3), 7, np.uint8)
    img[:, 8:] = 200
    out = nd.area_resize(img, 2, 3, 4.0)       # 3 cells of 4 over 10 columns: the third covers columns 8-9 only
    assert out.shape == (2, 3, 3)
    assert (out[:, 2] == 200).all() and (out[:, 0] == 7).all()


def test_keep_block_levels():
    grid = np.arange(0, 8).reshape(1, 8)
    kb = nd.keep_block_of(grid, 3)
    want = np.float32([0, 1 / 3, 2 / 3, 1, 1, 1, 1, 1])
    assert np.array_equal(kb[0], want)
    assert kb.dtype == np.float32 and kb[0, 0] == 0


@pytest.mark.parametrize("fmt", [nd.FMT_BGR, nd.FMT_YUV])
def test_flat_frame_gives_the_bilinear_image_of_the_median(fmt):
    # flat macroblocks: grid 0 -> keep 0 -> deblock 1: the region becomes (smooth * 1) / (1 + 1e-5), i.e. smooth
    rows, cols = 64, 96
    f = np.zeros((rows, cols, 3), np.uint8)
    f[...] = np.repeat(np.repeat(np.random.default_rng(1).integers(0, 256, (4, 6, 3)), 16, 0), 16, 1)
    out, info = nd.deblock(f, fmt)
    assert (info["grid"] == 0).all() and (info["keep"] == 0).all()
    assert np.array_equal(out, nd.resize_linear_u8(info["median"], rows, cols))


def test_strongly_deviating_blocks_are_returned_unchanged():
    # every block deviates by >= L from its mean: keep 1 everywhere -> deblock 0 -> src * 1 / (1 + 1e-5) rounds back to src
    rows, cols = 64, 64
    f = np.zeros((rows, cols, 3), np.uint8)
    f[::2] = 200
    out, info = nd.deblock(f, nd.FMT_YUV, detection_levels=5)
    assert (info["grid"] >= 5).all()
    assert np.array_equal(out, f)


def test_bytes_outside_the_region_are_untouched():
    f = np.clip(100 + np.random.default_rng(9).integers(-2, 3, (131, 67, 3)), 0, 255).astype(np.uint8)
    out, info = nd.deblock(f, nd.FMT_BGR, block_size=16)
    assert info["region"] == (0, 0, 64, 128)
    assert np.array_equal(out[128:], f[128:]) and np.array_equal(out[:, 64:], f[:, 64:])
    assert not np.array_equal(out[:128, :64], f[:128, :64])


@pytest.mark.parametrize("fmt", [nd.FMT_BGR, nd.FMT_YUV], ids=["bgr", "yuv"])
@pytest.mark.parametrize("case", [c for c in CASES if c[:2] != NOT_LIVE], ids=case_id)
def test_every_small_gpu_case_is_live(case, fmt):
    """A condition on the inputs of tests/test_deblock_gpu.py::test_small_and_edge_cases_bit_exact, not a measurement: the specification changes at
    least 25 % of the region's bytes and keep_block takes at least two values -- a case the filter leaves (nearly) unchanged would pass whatever the
    kernels do."""
    img, want, info = expected3(case, fmt)
    _, _, RW, RH = info["region"]
    changed = want[:RH, :RW] != img[:RH, :RW]
    assert changed.mean() >= 0.25, changed.mean()
    assert len(np.unique(info["keep_block"])) >= 2


def test_draw_influence_blends_magenta_where_the_filter_acts():
    f = np.full((32, 32, 3), 50, np.uint8)
    out, info = nd.deblock(f, nd.FMT_YUV)
    inf = nd.draw_influence(out, nd.FMT_YUV, info)
    assert (inf == np.uint8([105, 212, 234])).all()       # flat: keep 0 everywhere, all magenta


def test_too_small_frames_are_refused():
    with pytest.raises(ValueError):
        nd.deblock(np.zeros((15, 100, 3), np.uint8), nd.FMT_YUV)
    with pytest.raises(ValueError):
        nd.deblock(np.zeros((2, 2, 3), np.uint8), nd.FMT_YUV, block_size=2, filter_scaling=8.0)   # rint(0.25) = 0


def _declared(part):
    text = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    body = stable if part == 1 else experimental
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return set(re.findall(r"\b(lvk_hip_deblock_[a-z0-9_]+)\s*\(", body))


def test_header_declares_the_deblocking_abi():
    assert _declared(1) == {"lvk_hip_deblock_default_settings", "lvk_hip_deblock_create", "lvk_hip_deblock_configure",
                            "lvk_hip_deblock_destroy", "lvk_hip_deblock_apply", "lvk_hip_deblock_draw_influence",
                            "lvk_hip_deblock_filter_region"}
    assert _declared(2) == {"lvk_hip_deblock_get_grid"}
    text = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    assert int(re.search(r"#define LVK_HIP_ABI_VERSION (\d+)", text).group(1)) >= 7


def test_library_exports_the_deblocking_abi_and_its_defaults():
    from livevisionkit_amd import _native
    lib = _native.load()
    for name in sorted(_declared(1) | _declared(2)):
        assert hasattr(lib, name), name
    import livevisionkit_amd as lvk
    s = lvk.DeblockingFilterSettings()
    assert (s.detection_levels, s.block_size, s.filter_size, s.filter_scaling) == (3, 16, 5, 4.0)
    # a refused create reports through the context; without a context nothing is created
    out = ctypes.c_void_p()
    assert lib.lvk_hip_deblock_create(None, ctypes.byref(s), ctypes.byref(out)) != 0 and out.value is None
