"""CPU pins of the CAS specification (tests/np_cas.py) and of its C-ABI surface.

The restatement is held to the literals the FidelityFX arithmetic implies (host constant bit patterns, flat frames), to a float64 textbook
CAS as a bound, and its bit tricks to their exact functions over every float32 of the range CAS feeds them.  The header and the library
are checked for lvk_hip_cas / lvk_hip_cas_const; the host constant comes from the built library, so no device is needed."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import np_cas as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

PEAK_BITS = {0.0: 0xbe000000, 0.25: 0xbe0d3dcb, 0.5: 0xbe1d89d9, 0.8: 0xbe36db6e, 1.0: 0xbe4ccccd, 0.37: 0xbe149f07}


def _bits(v):
    return int(np.asarray(v, dtype=f32).view(np.uint32))


@pytest.mark.parametrize("sharpness", sorted(PEAK_BITS))
def test_peak_bit_patterns_of_the_specification(sharpness):
    assert _bits(nc.peak_of(sharpness)) == PEAK_BITS[sharpness]


@pytest.mark.parametrize("sharpness", sorted(PEAK_BITS))
def test_peak_bit_patterns_of_the_library(sharpness):
    from livevisionkit_amd import _native
    lib = _native.load()
    peak = ctypes.c_float()
    assert lib.lvk_hip_cas_const(f32(sharpness), ctypes.byref(peak)) == 0
    assert _bits(peak.value) == PEAK_BITS[sharpness]


def test_library_constant_clamps_and_refuses_nan():
    from livevisionkit_amd import _native
    lib = _native.load()
    peak = ctypes.c_float()
    for s, want in ((-3.0, 0.0), (7.5, 1.0)):
        assert lib.lvk_hip_cas_const(s, ctypes.byref(peak)) == 0 and _bits(peak.value) == PEAK_BITS[want]
    assert lib.lvk_hip_cas_const(float("nan"), ctypes.byref(peak)) != 0
    assert lib.lvk_hip_cas_const(0.5, None) != 0


def test_load_table_is_the_correctly_rounded_quotient():
    # u / 255 rounded to nearest float32 (ties cannot occur), and the kernel's q = u * (1/255) + fma(fma(-q, 255, u), 1/255, q) correction
    c = f32(1) / f32(255)
    wrong_by_multiply = 0
    for u in range(256):
        x = nc.UNIT[u]
        err = abs(Fraction(float(x)) - Fraction(u, 255))
        for nb in (np.nextafter(x, f32(-1)), np.nextafter(x, f32(2))):
            assert err < abs(Fraction(float(nb)) - Fraction(u, 255)), u
        q = f32(f32(u) * c)
        wrong_by_multiply += int(q != x)
        r = f32(Fraction(u) - Fraction(float(q)) * 255)                        # exact: |r| < 1 ulp of u, representable
        assert Fraction(float(r)) == Fraction(u) - Fraction(float(q)) * 255
        corrected = Fraction(float(r)) * Fraction(float(c)) + Fraction(float(q))  # one rounding of the exact value (fma)
        lo = f32(float(corrected))
        cands = [lo, np.nextafter(lo, f32(-1)), np.nextafter(lo, f32(2))]
        assert min(cands, key=lambda v: abs(Fraction(float(v)) - corrected)) == x, u
    assert wrong_by_multiply == 126


@pytest.mark.parametrize("sharpness", [0.0, 0.8, 1.0])
def test_flat_highlights_darken_by_one(sharpness):
    # med_rcp(1.0) = 0.99684685: a flat frame's centre e comes back scaled by it
    assert nc.med_rcp(f32(1)) == f32(0.99684685)
    for v, want in ((255, 254), (254, 253)):
        out = nc.cas(np.full((6, 7, 3), v, np.uint8), sharpness)
        assert (out == want).all(), (v, np.unique(out))


def test_flat_midtone_stays_and_flat_200_darkens_at_the_border():
    assert (nc.cas(np.full((9, 11, 3), 128, np.uint8)) == 128).all()
    out = nc.cas(np.full((9, 11, 3), 200, np.uint8))
    assert (out[1:-1, 1:-1] == 200).all()
    border = np.ones((9, 11), bool)
    border[1:-1, 1:-1] = False
    assert (out[border] == 199).all()
    assert (nc.cas(np.full((1, 1, 3), 77, np.uint8)) == 77).all()


def test_fourth_channel_is_written_as_255_and_does_not_take_part():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (23, 29, 4), dtype=np.uint8)
    out = nc.cas(img, 0.6)
    assert (out[..., 3] == 255).all()
    assert np.array_equal(out[..., :3], nc.cas(img[..., :3], 0.6))


@pytest.mark.parametrize("perm", [(2, 1, 0), (1, 2, 0), (0, 2, 1)])
def test_channel_permutation_permutes_the_output(perm):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (31, 37, 3), dtype=np.uint8)
    assert np.array_equal(nc.cas(img[..., list(perm)], 0.37), nc.cas(img, 0.37)[..., list(perm)])


def _smooth(rows, cols, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols] / np.array([rows, cols]).reshape(2, 1, 1)
    chans = [np.sin(x * rng.uniform(2, 9) + y * rng.uniform(2, 9) + rng.uniform(0, 6)) for _ in range(3)]
    return np.clip(np.rint(127.5 + 120 * np.stack(chans, -1)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("content", ["random", "smooth"])
@pytest.mark.parametrize("sharpness", [0.0, 0.37, 0.8, 1.0])
def test_bounded_by_the_textbook_cas(content, sharpness):
    img = np.random.default_rng(5).integers(0, 256, (120, 160, 3), dtype=np.uint8) if content == "random" else _smooth(120, 160, 5)
    d = np.abs(nc.cas(img, sharpness).astype(int) - nc.textbook_cas(img, sharpness).astype(int))
    assert d.max() <= 12 and d.mean() <= 0.6, (d.max(), d.mean())


def test_approximation_is_not_the_textbook_cas():
    img = np.random.default_rng(5).integers(0, 256, (120, 160, 3), dtype=np.uint8)
    assert not np.array_equal(nc.cas(img, 1.0), nc.textbook_cas(img, 1.0))


def test_bit_trick_relative_errors_over_every_float32_in_range():
    lo, hi = _bits(f32(2.0 ** -10)), _bits(f32(2.0))
    worst = {"rcp": 0.0, "sqrt": 0.0, "med": 0.0}
    for start in range(lo, hi + 1, 1 << 23):
        u = np.arange(start, min(start + (1 << 23), hi + 1), dtype=np.uint32)
        v = u.view(f32)
        v64 = v.astype(np.float64)
        worst["rcp"] = max(worst["rcp"], float(np.max(np.abs(nc.lo_rcp(v).astype(np.float64) * v64 - 1))))
        worst["sqrt"] = max(worst["sqrt"], float(np.max(np.abs(nc.lo_sqrt(v).astype(np.float64) / np.sqrt(v64) - 1))))
        worst["med"] = max(worst["med"], float(np.max(np.abs(nc.med_rcp(v).astype(np.float64) * v64 - 1))))
    assert worst["rcp"] <= 0.061 and worst["sqrt"] <= 0.041 and worst["med"] <= 0.0032, worst
    assert worst["rcp"] > 0.05 and worst["sqrt"] > 0.03 and worst["med"] > 0.003, worst      # the approximations, not exact functions


# ---- the C-ABI surface -----------------------------------------------------------------------------------------------------------

def _header():
    return open(os.path.join(ROOT, "include", "lvk_hip.h")).read()


def test_header_declares_the_cas_abi():
    text = _header()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    assert re.search(r"int\s+lvk_hip_cas\(lvk_hip_ctx\* ctx, const void\* d_src, int src_step, int rows, int cols, int format, void\* d_dst, "
                     r"int dst_step, float sharpness\);", stable)
    assert "lvk_hip_cas(" not in experimental
    assert "int lvk_hip_cas_const(float sharpness, float* peak);" in experimental and "lvk_hip_cas_const(" not in stable
    assert int(re.search(r"#define LVK_HIP_ABI_VERSION (\d+)", text).group(1)) >= 8


def test_library_reports_abi_8_and_refuses_without_a_context():
    from livevisionkit_amd import _native
    lib = _native.load()
    assert lib.lvk_hip_abi_version() >= 8
    assert b"ABI %d" % lib.lvk_hip_abi_version() in lib.lvk_hip_version()
    assert lib.lvk_hip_cas(None, None, 3, 1, 1, 0, None, 3, ctypes.c_float(0.5)) != 0


def test_python_binding_is_exported():
    import livevisionkit_amd as lvk
    assert "CASFilter" in lvk.__all__
    from livevisionkit_amd.cas import cas_const
    assert _bits(cas_const(0.8)) == PEAK_BITS[0.8]
