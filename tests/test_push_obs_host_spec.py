"""lvk_hip_stab_push_obs_host at the boundary, without a device: the symbol, its place in PART 1 of include/lvk_hip.h (ABI 12), the header as
pedantic C99 with a call of the new entry in it, the ctypes prototype, a NULL filter, and the plane shapes host_planes_obs documents."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lvk_hip.h")
FORMATS12 = ["I422", "I42A", "I444", "YUVA", "YUY2", "YVYU", "UYVY", "AYUV", "BGR3", "RGBA", "BGRA", "BGRX"]


def test_symbol_is_exported_and_declared_in_part_1():
    from livevisionkit_amd import _native
    lib = _native.load()
    assert hasattr(lib, "lvk_hip_stab_push_obs_host")
    text = open(HEADER).read()
    stable, experimental = text.split("PART 2 -- EXPERIMENTAL / DIAGNOSTICS  (no ABI promise")
    assert "lvk_hip_stab_push_obs_host(" in stable and "lvk_hip_stab_push_obs_host(" not in experimental
    decl = (r"int\s+lvk_hip_stab_push_obs_host\(lvk_hip_stab\* stab, int video_format,\s*const void\* const h_planes\[3\], const int steps\[3\], int rows, int cols, "
            r"uint64_t timestamp,\s*void\* const oh_planes\[3\], const int o_steps\[3\], int o_rows,\s*int\* produced, uint64_t\* out_timestamp, "
            r"lvk_frame_info\* emitted\);")
    assert re.search(decl, stable), "the declaration differs from the issue's"
    # the header says that look-ahead is out of scope for these formats
    comment = stable[:stable.index("lvk_hip_stab_push_obs_host(lvk_hip_stab* stab")]
    assert "LOOK-AHEAD is out of scope" in comment[-4000:]


def test_header_and_library_agree_on_abi_12():
    from livevisionkit_amd import _native
    lib = _native.load()
    want = int(re.search(r"#define LVK_HIP_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert want >= 12 and lib.lvk_hip_abi_version() == want
    assert ("ABI %d" % want).encode() in lib.lvk_hip_version()


def test_header_with_the_new_entry_is_pedantic_c99(tmp_path):
    import torch
    src = tmp_path / "obs_host.c"
    src.write_text('#include "lvk_hip.h"\n'
                   'int main(void) {\n'
                   '  const void* in[3] = {0, 0, 0}; void* out[3] = {0, 0, 0}; int steps[3] = {0, 0, 0}; int produced = 7; uint64_t ts = 0; lvk_frame_info info = {0, 0, 0};\n'
                   '  int rc = lvk_hip_stab_push_obs_host(0, LVK_VIDEO_FORMAT_UYVY, in, steps, 2, 2, 0, out, steps, 2, &produced, &ts, &info);\n'
                   '  return (rc == LVK_HIP_ERR_ARG && lvk_hip_abi_version() == LVK_HIP_ABI_VERSION && LVK_HIP_ABI_VERSION >= 12) ? 0 : 1; }\n')
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib")
    exe = str(tmp_path / "obs_host")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + os.path.join(ROOT, "livevisionkit_amd"), "-llvk_hip", "-L" + tlib, "-l:libamdhip64.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "livevisionkit_amd"), "-Wl,-rpath," + tlib])
    assert subprocess.run([exe]).returncode == 0


def test_native_declares_the_prototype():
    from livevisionkit_amd import _native
    assert "lvk_hip_stab_push_obs_host" in _native.symbols()
    lib = _native.load()
    fn = lib.lvk_hip_stab_push_obs_host
    P = ctypes.c_void_p
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [P, ctypes.c_int, P * 3, ctypes.c_int * 3, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, P * 3, ctypes.c_int * 3, ctypes.c_int,
                                 ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64), P]


def test_null_filter_is_an_argument_error_without_a_device():
    from livevisionkit_amd import _native
    lib = _native.load()
    planes = (ctypes.c_void_p * 3)(); steps = (ctypes.c_int * 3)(8, 0, 0)
    produced = ctypes.c_int(5); ts = ctypes.c_uint64(0)
    for vf in (5, 1, 9, 99):                                    # UYVY, I420 (the delegate), Y800, unknown
        rc = lib.lvk_hip_stab_push_obs_host(None, vf, planes, steps, 2, 2, 0, planes, steps, 2, ctypes.byref(produced), ctypes.byref(ts), None)
        assert rc == -1, vf                                     # LVK_HIP_ERR_ARG
    assert int(re.search(r"#define LVK_HIP_ERR_ARG\s+(-?\d+)", open(HEADER).read()).group(1)) == -1


@pytest.mark.parametrize("pitch_extra", [0, 13, 64])
@pytest.mark.parametrize("fmt", FORMATS12 + ["I420", "I40A", "NV12"])
def test_host_planes_obs_shapes(fmt, pitch_extra, monkeypatch):
    """host_planes_obs(fmt, rows, cols, pitch_extra): the documented shapes, rows pitch_extra bytes apart beyond their pixels, one block, in order.
    (The pinned allocation is replaced by host memory here: no device.)"""
    import numpy as np
    import livevisionkit_amd as lvk
    rows, cols = 6, 8
    want = {"I422": [(6, 8), (6, 4), (6, 4)], "I42A": [(6, 8), (6, 4), (6, 4)], "I444": [(6, 8)] * 3, "YUVA": [(6, 8)] * 3,
            "YUY2": [(6, 8, 2)], "YVYU": [(6, 8, 2)], "UYVY": [(6, 8, 2)], "AYUV": [(6, 8, 4)], "BGR3": [(6, 8, 3)],
            "RGBA": [(6, 8, 4)], "BGRA": [(6, 8, 4)], "BGRX": [(6, 8, 4)],
            "I420": [(6, 8), (3, 4), (3, 4)], "I40A": [(6, 8), (3, 4), (3, 4)], "NV12": [(6, 8), (3, 4, 2)]}[fmt]
    assert lvk.StabilizationFilter.obs_plane_shapes(fmt, rows, cols) == want
    with pytest.raises(ValueError):
        lvk.StabilizationFilter.obs_plane_shapes("Y800", rows, cols)
    keep = []

    class FakeLib:
        @staticmethod
        def lvk_hip_host_malloc(ctx, n, ref):
            buf = (ctypes.c_uint8 * n)(); keep.append((buf, n))
            ctypes.cast(ref, ctypes.POINTER(ctypes.c_void_p))[0] = ctypes.addressof(buf)
            return 0

    class FakeCtx:
        handle = None
        VIDEO_FORMATS = lvk.Context.VIDEO_FORMATS

        @staticmethod
        def _check(rc):
            assert rc == 0

    f = object.__new__(lvk.StabilizationFilter)
    f.lib, f.ctx = FakeLib, FakeCtx
    planes = f.host_planes_obs(fmt, rows, cols, pitch_extra)
    assert [p.shape for p in planes] == want
    base = ctypes.addressof(keep[0][0]); off = 0
    for p, sh in zip(planes, want):
        rowb = sh[1] * (sh[2] if len(sh) == 3 else 1)
        assert p.dtype == np.uint8 and p.strides[0] == rowb + pitch_extra and p.strides[-1] == 1
        assert p.ctypes.data == base + off
        off += sh[0] * (rowb + pitch_extra)
    assert off == keep[0][1]
    for i, p in enumerate(planes):                              # writable views of the block, not copies
        p[...] = i + 1
    assert np.frombuffer(keep[0][0], np.uint8).max() == len(planes)
    a = f.prepare_obs_host(fmt, planes)
    assert a["vf"].value == lvk.Context.VIDEO_FORMATS[fmt] and (a["rows"].value, a["cols"].value) == (rows, cols)
    assert list(a["steps"])[:len(planes)] == [p.strides[0] for p in planes] and a["ptrs"][0] == base
    f._host_blocks = []                                         # (nothing of the fake allocator reaches lvk_hip_host_free)
    f.handle = None
