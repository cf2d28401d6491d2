"""CPU pins of CAS and FSR EASU on one-channel frames.  Neither filter has a one-channel program in the reference, so
both are DEFINED through the three-channel specifications (tests/np_cas.py, tests/np_fsr.py) on (g, g, g); tests/ffx_gray_cases.py holds the
definitions and the cases.  Checked here, without a device: the premises of the definitions (on grey input the three channels of either
specification are equal, EASU's result does not depend on the format, a grey texel's luma is exactly twice its value), that every case the
device runs changes its input (a kernel that copied, or one that picked the nearest texel, would fail the GPU test), and the surface: the
three entries in the header, the library and the binding, and the host's choice between the two EASU paths."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import ffx_gray_cases as fc
from tests import np_cas as nc
from tests import np_fsr as nf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["lvk_hip_cas_gray", "lvk_hip_fsr_easu_gray", "lvk_hip_fsr_easu_gray_path"]
f32 = np.float32


def _lib():
    from livevisionkit_amd import _native
    return _native.load()


@pytest.mark.parametrize("rows,cols", [(3, 5), (17, 65), (45, 77)])
def test_cas_of_grey_input_has_equal_channels(rows, cols):
    g = fc.frame(rows, cols, seed=rows + cols)
    for s in fc.SHARPNESS:
        out = nc.cas(fc.grey3(g), s)
        assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2]), s


@pytest.mark.parametrize("rows,cols,region,oh,ow", [(45, 77, (0, 0, 77, 45), 90, 154), (40, 57, (37, 25, 20, 15), 31, 17),
                                                    (3, 5, (0, 0, 5, 3), 7, 11), (60, 100, (0, 0, 100, 60), 30, 50)])
def test_easu_of_grey_input_has_equal_channels_in_every_format(rows, cols, region, oh, ow):
    g = fc.centred(rows, cols, seed=oh)
    outs = [nf.fsr(fc.grey3(g), fmt, region, oh, ow) for fmt in (fc.BGR, fc.RGB, fc.YUV)]
    for out in outs:
        assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
        assert np.array_equal(out, outs[0])
    assert np.array_equal(fc.fsr_gray(g, region, oh, ow), outs[0][..., 0])


def test_the_luma_of_a_grey_texel_is_exactly_twice_its_value():
    """0.5 v + (0.5 v + v) in binary32 for the 256 values a byte loads as: k_fsr_easu_gray forms it as v + v."""
    v = nc.UNIT[np.arange(256, dtype=np.uint8)]
    assert v.dtype == f32
    assert np.array_equal(nf.luma(v, v, v), v + v)
    assert np.array_equal(v * f32(0.5) + (v * f32(0.5) + v), f32(2.0) * v)


def test_every_cas_case_of_the_device_test_is_live():
    seen = 0
    for case, sharpness in fc.cas_live_cases():
        g, want = fc.cas_expected(case, sharpness)
        assert want.shape == g.shape and want.dtype == np.uint8
        if g.size >= fc.LIVE_PIXELS:
            seen += 1
            assert (want != g).mean() >= fc.LIVE, (case, sharpness, (want != g).mean())
    assert seen >= 80


def test_every_easu_case_of_the_device_test_is_live():
    seen = 0
    for case in fc.fsr_cases():
        rows, cols, _, region, oh, ow, _ = case
        g, want = fc.fsr_expected(*case)
        assert want.shape == (oh, ow) and want.dtype == np.uint8
        if region[2] * region[3] >= fc.LIVE_PIXELS and oh * ow >= fc.LIVE_PIXELS:
            seen += 1
            share = (want != fc.nearest(g, region, oh, ow)).mean()
            assert share >= fc.LIVE, (case, share)
    assert seen >= 25


def test_the_library_exports_and_the_header_declares_the_three_entries():
    header = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    from livevisionkit_amd import _native
    lib = _lib()
    experimental = header.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")[1]
    for sym in SYMBOLS:
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", experimental)
        assert m, f"{sym} is not declared in PART 2 of include/lvk_hip.h"
        assert hasattr(lib, sym), f"{sym} is not exported by liblvk_hip.so"
        restype, argtypes = _native._SIG[sym]
        assert restype is ctypes.c_int and len(argtypes) == len(m.group(1).split(",")), sym
    # refused without a context, like their three-channel siblings
    region = (ctypes.c_int * 4)(0, 0, 1, 1)
    assert lib.lvk_hip_cas_gray(None, None, 1, 1, 1, None, 1, ctypes.c_float(0.5)) != 0
    assert lib.lvk_hip_fsr_easu_gray(None, None, 1, 1, 1, region, None, 1, 1, 1) != 0


def test_the_gray_easu_path_is_a_host_function_with_a_larger_staged_budget():
    """A staged one-channel texel is 4 bytes against 16: every scale the three-channel kernel stages stays staged, a 2x downscale joins them,
    and the lists of the device test cover both paths."""
    lib = _lib()
    paths = set()
    for region, oh, ow in fc.STAGED_3 + fc.DIRECT_3:
        p3, p1 = lib.lvk_hip_fsr_easu_path(region[2], region[3], oh, ow), lib.lvk_hip_fsr_easu_gray_path(region[2], region[3], oh, ow)
        assert p1 in (0, 1) and p1 <= p3, (region, oh, ow)
        paths.add(p1)
    assert paths == {0, 1}
    assert lib.lvk_hip_fsr_easu_gray_path(1920, 1080, 2160, 3840) == 0          # upscale: staged
    assert lib.lvk_hip_fsr_easu_gray_path(3840, 2160, 1080, 1920) == 0          # 2x downscale: staged (direct with three channels)
    assert lib.lvk_hip_fsr_easu_gray_path(3840, 2160, 270, 480) == 1            # 8x downscale: direct
    assert lib.lvk_hip_fsr_easu_gray_path(1, 1, 1, 1) == 0
    assert lib.lvk_hip_fsr_easu_gray_path(0, 1, 1, 1) < 0 and lib.lvk_hip_fsr_easu_gray_path(1, 1, 1, -1) < 0
