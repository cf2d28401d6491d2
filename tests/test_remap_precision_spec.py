"""LVK_REMAP_1LSB without a device: its specification (tests/np_easu_1lsb.py) against the exact EASU of tests/np_easu.py, the instruction and register
figures of the `_r1` kernels read from the gfx950 assembly, and the four new symbols at the boundary.

The bounds are those the mode is defined by: every byte within 1 of the exact output (SURVEY.md section 8c's tolerance for the remap row) and at most
1e-4 of the bytes different at all -- the second one so that a sloppier regrouping (colours kept in 0 .. 255: up to 22 LSB on edges, 0.1 % of the bytes
different) cannot pass as "within 1"."""
import os
import re

import numpy as np
import pytest

from tests import np_easu, np_easu_1lsb
from tests.isa import assemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = 97, 131
# one mild perspective matrix (dst -> src): a little rotation, shear, shift and a perspective term that keeps the whole frame's denominator near 1
H_MILD = [1.012, 0.021, -1.7, -0.017, 0.991, 2.3, 2.1e-5, -1.6e-5, 1.0]
MAX_DIFF, MAX_SHARE = 1, 1e-4


def textures():
    rng = np.random.default_rng(20)
    yy, xx = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    ch = np.arange(3)[None, None, :]
    sin = 127.5 + 100.0 * np.sin(xx[..., None] * (0.11 + 0.03 * ch) + yy[..., None] * (0.07 - 0.02 * ch) + ch)
    out = {}
    out["noise"] = rng.integers(0, 256, (ROWS, COLS, 3))
    out["sinusoid"] = sin
    out["slanted_edges"] = np.where(((xx * 0.8 + yy * 0.45) % 23.0 < 11.0)[..., None], np.array([228, 40, 190]), np.array([18, 215, 66]))
    out["checker3"] = np.where((((xx // 3) + (yy // 3)) % 2 == 0)[..., None], np.array([240, 128, 30]), np.array([12, 120, 220]))
    out["sinusoid_noise"] = sin + rng.normal(0.0, 6.0, (ROWS, COLS, 3))
    out["flat_pm1"] = 128 + rng.integers(-1, 2, (ROWS, COLS, 3))
    # a ramp whose pseudo-luma 0.5 c0 + c1 + 0.5 c2 is nearly constant: the direction analysis works on rounding noise
    r = np.round(40.0 + 160.0 * xx / (COLS - 1))
    out["ramp_flat_luma"] = np.stack([r, 200.0 - r, r], axis=-1) + rng.integers(0, 2, (ROWS, COLS, 3))
    return {k: np.clip(np.round(v), 0, 255).astype(np.uint8) for k, v in out.items()}


def test_spec_is_within_one_lsb_of_the_exact_easu_and_almost_everywhere_equal():
    total = differing = 0
    worst = 0
    bg = (16, 128, 128)
    for name, src in textures().items():
        for yuv in (True, False):
            exact = np_easu.remap_homography(src, H_MILD, bg, yuv)
            got, ea = np_easu_1lsb.remap_tail(src, *np_easu_1lsb.homography_coords(ROWS, COLS, H_MILD), bg, yuv)
            assert ea.mean() > 0.85, "the matrix is meant to keep most of the frame on the EASU path"
            d = np.abs(got.astype(np.int16) - exact.astype(np.int16))
            print(f"{name:16s} yuv={int(yuv)}: max |diff| {int(d.max())}, {int((d != 0).sum())} of {d.size} bytes differ")
            assert np.array_equal(got[~ea], exact[~ea]), f"{name}: a border-band or background byte differs"
            worst = max(worst, int(d.max())); differing += int((d != 0).sum()); total += d.size
    print(f"all: max |diff| {worst}, {differing} of {total} bytes differ ({differing / total:.2e})")
    assert total == 7 * 2 * ROWS * COLS * 3
    assert worst <= MAX_DIFF
    assert differing <= MAX_SHARE * total, f"{differing} of {total} bytes differ"


def _bodies_of(code, kernel):
    return {m.group(1): m.group(2) for m in re.finditer(r"^(\S*" + kernel + r"I\S*):[^\n]*\n(.*?)\.Lfunc_end", code, re.S | re.M)}


def _valu_of(body):
    ops = [ln.split()[0] for ln in body.splitlines() if ln.strip() and not ln.strip().startswith((";", ".", "//")) and not ln.strip().endswith(":")]
    return [o for o in ops if o.startswith("v_")]


@pytest.mark.parametrize("kernel,ceiling", [("k_remap_homography_420", 2066), ("k_remap_mesh_420", 2 * 2200)])
def test_one_lsb_twins_issue_seven_percent_fewer_valu_within_the_register_budget(kernel, ceiling):
    """The `_r1` twins of the fused 4:2:0 kernels exist (I420 and NV12), use no scratch and at most 80 VGPRs -- the persistent grid of the overlap mode
    depends on that budget (tests/test_isa_budget.py) --, and issue at least 7 % fewer static VALU instructions than the exact kernel assembled in the
    same run (the regrouping saves 15 per tap stage, 8.8 % of the thread; the slack is for compiler scheduling).  The exact kernels stay within the
    ceilings of tests/test_isa_budget.py."""
    code, kernels = assemble("remap")
    exact, twins = _bodies_of(code, kernel), _bodies_of(code, kernel + "_r1")
    assert len(exact) == 2 and len(twins) == 2, (list(exact), list(twins))
    for name in twins:
        scratch, vgprs = kernels[name]
        assert scratch == 0 and vgprs <= 80, f"{name}: {scratch} bytes of scratch, {vgprs} VGPRs"
    for (en, eb), (tn, tb) in zip(sorted(exact.items()), sorted(twins.items())):
        ne, nt = len(_valu_of(eb)), len(_valu_of(tb))
        print(f"{kernel}: exact {ne}, 1-LSB {nt} static VALU ({100.0 * (ne - nt) / ne:.1f} % fewer); VGPRs {kernels[en][1]} / {kernels[tn][1]}")
        assert ne <= ceiling, f"{en}: {ne} static VALU instructions (ceiling {ceiling})"
        assert nt <= 0.93 * ne, f"{tn}: {nt} static VALU instructions against {ne} of the exact kernel"


def test_every_covered_kernel_has_a_twin_and_the_uncovered_ones_have_none():
    names = set()
    for unit in ("remap", "remap_obs", "remap_px"):
        names |= {re.search(r"\d+(k_\w+?)I", k).group(1) for k in assemble(unit)[1] if re.search(r"\d+(k_\w+?)I", k)}
    exact = {n for n in names if not n.endswith("_r1")}
    for n in exact:
        covered = n.startswith("k_remap_") and not n.endswith("_px")        # `_px`: the one- and four-channel kernels (remap_px.hip)
        assert ((n + "_r1") in names) == covered, n
    assert "k_easu_scale" in exact and "k_remap_homography_planes" in exact and {"k_remap_homography_px", "k_remap_mesh_px", "k_remap_map_px"} <= exact


def test_boundary_carries_the_four_symbols():
    from livevisionkit_amd import _native
    header = open(os.path.join(ROOT, "include", "lvk_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stable = header.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")[0]
    lib = _native.load()
    for name in ("lvk_hip_set_remap_precision", "lvk_hip_get_remap_precision", "lvk_hip_stab_set_remap_precision", "lvk_hip_stab_get_remap_precision"):
        assert name + "(" in stable, name
        assert name in _native.symbols() and hasattr(lib, name), name
        assert name in doc, name
    assert re.search(r"#define LVK_REMAP_EXACT 0\b", header) and re.search(r"#define LVK_REMAP_1LSB  ?1\b", header)
    # an unknown value is refused without a device as well, and a NULL handle is an argument error
    assert lib.lvk_hip_set_remap_precision(None, 1) == -1 and lib.lvk_hip_stab_set_remap_precision(None, 1) == -1
    assert lib.lvk_hip_get_remap_precision(None) == -1 and lib.lvk_hip_stab_get_remap_precision(None) == -1


def test_cpp_facade_driver_compiles(tmp_path):
    """lvk::RemapPrecision, StabilizationFilter::set_remap_precision and hip::Context::set_remap_precision against the headers alone"""
    from tests.facade import build_facade
    build_facade(tmp_path, os.path.join(ROOT, "tests", "cpp", "remap_precision_facade.cpp"))


def test_no_compile_time_tolerance_switch_is_left():
    flag = "LVK_EASU_TOLERANT"
    hits = []
    for base in (os.path.join("livevisionkit_amd", "csrc"), "scripts"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if flag in open(os.path.join(dirpath, f), errors="ignore").read():
                    hits.append(os.path.join(dirpath, f))
    assert not hits, hits
