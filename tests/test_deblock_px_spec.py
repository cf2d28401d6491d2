"""CPU pins of the one- and four-channel deblocking specification (tests/np_deblock_px.py) and of its C-ABI surface.

The specification is a composition of the three-channel restatement's channel-generic steps, so it is held to that restatement (which
tests/test_deblock_spec.py holds to scipy and the oracle) through three identities, its median to scipy once more at one and four channels, and every
GPU case to a liveness condition: a case the filter leaves (nearly) unchanged would pass whatever the kernels do."""
import os
import re

import numpy as np
import pytest

from tests import np_convert as nc
from tests import np_deblock as nd
from tests import np_deblock_px as npx
from tests.deblock_px_cases import BGRA, CASES, GRAY, NAMES, NOT_LIVE, RGBA, VARIANTS, case_id, expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gray_is_channel_0_of_the_three_channel_filter_on_the_replicated_frame(case):
    img, want, info = expected(case, GRAY)
    out3, info3 = nd.deblock(np.repeat(img[..., None], 3, axis=2), nd.FMT_YUV, *case[2:6])
    assert np.array_equal(want, out3[..., 0])
    assert info["region"] == info3["region"] and np.array_equal(info["keep_block"], info3["keep_block"])


@pytest.mark.parametrize("fmt", [BGRA, RGBA], ids=[NAMES[BGRA], NAMES[RGBA]])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_colour_bytes_are_the_three_channel_filter_and_the_grey_is_np_converts(case, fmt):
    img, want, info = expected(case, fmt)
    fmt3 = nd.FMT_BGR if fmt == BGRA else nd.FMT_RGB
    out3, info3 = nd.deblock(np.ascontiguousarray(img[..., :3]), fmt3, *case[2:6])
    assert np.array_equal(want[..., :3], out3)
    assert np.array_equal(info["mean"], info3["mean"]) and np.array_equal(info["grid"], info3["grid"])
    grey = nc.reformat(img, fmt, nc.GRAY)
    assert np.array_equal(grey.reshape(img.shape[:2]), npx.gray_px(img, fmt))


def test_alpha_is_filtered_like_a_colour_channel():
    # the alpha plane alone, as the one channel of a frame whose keep map is the four-channel frame's, gives the four-channel result's byte 3:
    # checked through the steps that do not involve the grey
    img, want, info = expected(CASES[0], BGRA)
    _, _, RW, RH = info["region"]
    a = img[:RH, :RW, 3]
    hs, ws = info["small"].shape[:2]
    small = nd.area_resize(a, hs, ws, 1.0 / float(nd.f32(1) / nd.f32(CASES[0][5])))
    smooth = nd.resize_linear_u8(nd.median(small[..., None], CASES[0][4]), RH, RW)
    assert np.array_equal(nd.blend(a[..., None], smooth, info["keep"])[..., 0], want[:RH, :RW, 3])
    assert np.array_equal(want[RH:], img[RH:]) and np.array_equal(want[:, RW:], img[:, RW:])


@pytest.mark.parametrize("k", [3, 5, 7, 9])
@pytest.mark.parametrize("channels", [1, 4])
def test_median_is_scipy_median_filter_nearest(channels, k):
    ndimage = pytest.importorskip("scipy.ndimage")
    img = np.random.default_rng(10 * k + channels).integers(0, 256, (37, 53, channels), dtype=np.uint8)
    got = nd.median(img, k)
    for c in range(channels):
        assert np.array_equal(got[..., c], ndimage.median_filter(img[..., c], size=k, mode="nearest")), c


@pytest.mark.parametrize("fmt", VARIANTS, ids=[NAMES[v] for v in VARIANTS])
@pytest.mark.parametrize("case", [c for c in CASES if c[:2] != NOT_LIVE], ids=case_id)
def test_every_gpu_case_is_live(case, fmt):
    """A condition on the test inputs, not a measurement: the specification changes at least 25 % of the region's bytes (of a four-channel frame's
    alpha bytes as well) and keep_block takes at least two values."""
    img, want, info = expected(case, fmt)
    _, _, RW, RH = info["region"]
    changed = want[:RH, :RW] != img[:RH, :RW]
    assert changed.mean() >= 0.25, changed.mean()
    if fmt != GRAY:
        assert changed[..., 3].mean() >= 0.25, changed[..., 3].mean()
    assert len(np.unique(info["keep_block"])) >= 2


def test_refused_shapes_raise():
    with pytest.raises(ValueError):
        npx.deblock_px(np.zeros((15, 100), np.uint8), GRAY)
    with pytest.raises(ValueError):
        npx.deblock_px(np.zeros((2, 2, 4), np.uint8), BGRA, block_size=2, filter_scaling=8.0)
    with pytest.raises(ValueError):
        npx.deblock_px(np.zeros((32, 32, 3), np.uint8), BGRA)
    with pytest.raises(ValueError):
        npx.deblock_px(np.zeros((32, 32, 4), np.uint8), GRAY)


SYMBOLS = {"lvk_hip_deblock_apply_gray": "lvk_hip_deblock* deb, void* d_frame, int step, int rows, int cols, int region_xywh[4]",
           "lvk_hip_deblock_apply_c4": "lvk_hip_deblock* deb, void* d_frame, int step, int rows, int cols, int format, int region_xywh[4]"}


def test_header_and_bindings_declare_the_two_entries():
    """include/lvk_hip_deblock_px.h declares exactly the two entries, lvk_hip.h includes it (inside its include guard, behind its own declarations), and
    livevisionkit_amd/_native.py binds exactly what it declares -- the rule tests/test_abi.py holds lvk_hip.h to."""
    import ctypes
    from livevisionkit_amd import _native
    text = open(os.path.join(ROOT, "include", "lvk_hip_deblock_px.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(re.findall(r"\b(lvk_(?:hip|stab)_[a-z0-9_]+)\s*\(", code)) == sorted(SYMBOLS) == _native.symbols_deblock_px()
    main = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    experimental = main.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")[1]
    assert re.search(r'^#include "lvk_hip_deblock_px.h".*\n#endif /\* LVK_HIP_H \*/\s*$', experimental, re.M)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _native.load()
    for name, args in SYMBOLS.items():
        assert re.search(r"^int\s+%s\(%s\);" % (name, re.escape(args)), code, re.M), name
        assert name in doc and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == args.count(",") + 1
    # a NULL handle is refused before anything is touched
    assert lib.lvk_hip_deblock_apply_gray(None, None, 0, 0, 0, None) != 0
    assert lib.lvk_hip_deblock_apply_c4(None, None, 0, 0, 0, BGRA, None) != 0


def test_the_header_is_plain_c_either_way_round(tmp_path):
    """C99 with -pedantic, whichever of the two headers a host includes first."""
    import subprocess
    for first, second in (("lvk_hip.h", "lvk_hip_deblock_px.h"), ("lvk_hip_deblock_px.h", "lvk_hip.h")):
        src = tmp_path / "px.c"
        src.write_text('#include "%s"\n#include "%s"\n'
                       'int main(void) { (void)lvk_hip_deblock_apply_gray; (void)lvk_hip_deblock_apply_c4; (void)lvk_hip_deblock_apply; return 0; }\n' % (first, second))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
