"""ctypes wrapper around oracle/_ref/libffx_ref.so: the OBS plugin's own CAS and FSR shader text (cas.effect, fsr.effect and the FidelityFX
headers they include) and its host constants (CasSetup, FsrEasuCon), compiled for the host by `make -C oracle ref`.  TEST INFRASTRUCTURE
ONLY.  libffx_ref_f32lit.so is the same text with every unsuffixed literal typed as float (HLSL's reading)."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
LIB = os.path.join(REF_DIR, "libffx_ref.so")
LIB_F32LIT = os.path.join(REF_DIR, "libffx_ref_f32lit.so")

_c = ctypes
_f32p = _c.POINTER(_c.c_float)
_u32p = _c.POINTER(_c.c_uint32)
_i32p = _c.POINTER(_c.c_int)
f32 = np.float32


def _p(a, t):
    return a.ctypes.data_as(t)


class FfxRef:
    def __init__(self, path):
        L = self.lib = _c.CDLL(path)
        L.ffx_ref_cas_unit.restype = _c.c_int
        L.ffx_ref_cas_unit.argtypes = [_f32p, _c.c_int, _c.c_int, _c.c_float, _f32p]
        L.ffx_ref_easu_unit.restype = _c.c_int
        L.ffx_ref_easu_unit.argtypes = [_f32p, _f32p, _f32p, _c.c_int, _c.c_int, _i32p, _c.c_int, _c.c_int, _f32p, _f32p, _f32p]
        L.ffx_ref_cas_setup.restype = None
        L.ffx_ref_cas_setup.argtypes = [_c.c_float, _u32p]
        L.ffx_ref_easu_con.restype = None
        L.ffx_ref_easu_con.argtypes = [_c.c_float] * 6 + [_u32p]

    def cas_setup(self, sharpness):
        """const1 of CasSetup(const0, const1, sharpness, 0, 0, 0, 0), CASEffect::configure's call: 4 uint32 words."""
        out = np.zeros(4, np.uint32)
        self.lib.ffx_ref_cas_setup(f32(sharpness), _p(out, _u32p))
        return out

    def peak(self, sharpness):
        return self.cas_setup(sharpness)[:1].view(f32)[0]

    def easu_con(self, rw, rh, W, H, ow, oh):
        """con0..con3 of FsrEasuCon with FSREffect::configure's argument list: 16 float32 values."""
        out = np.zeros(16, np.uint32)
        self.lib.ffx_ref_easu_con(f32(rw), f32(rh), f32(W), f32(H), f32(ow), f32(oh), _p(out, _u32p))
        return out.view(f32)

    def cas_unit(self, x, peak):
        """cas.effect's PSMain over a float32 [rows, cols, 3] frame: float32 [rows, cols, 4], the shader's float4 as it returns it."""
        x = np.ascontiguousarray(x, f32)
        rows, cols, ch = x.shape
        assert ch == 3
        out = np.empty((rows, cols, 4), f32)
        rc = self.lib.ffx_ref_cas_unit(_p(x, _f32p), rows, cols, f32(peak), _p(out, _f32p))
        assert rc == 0, "ffx_ref_cas_unit: %d" % rc
        return out

    def easu_unit(self, r, g, b, region, out_rows, out_cols, con=None):
        """fsr.effect's EASUPSMain over float32 [H, W] planes: (float32 [out_rows, out_cols, 4], the largest distance of a sampled
        u W / v H from a texel centre).  con defaults to the reference's own FsrEasuCon of the sizes."""
        r, g, b = (np.ascontiguousarray(p, f32) for p in (r, g, b))
        H, W = r.shape
        assert g.shape == (H, W) and b.shape == (H, W)
        if con is None:
            con = self.easu_con(region[2], region[3], W, H, out_cols, out_rows)
        con = np.ascontiguousarray(con, f32)
        reg = (_c.c_int * 4)(*region)
        out = np.empty((out_rows, out_cols, 4), f32)
        dev = _c.c_float(-1.0)
        rc = self.lib.ffx_ref_easu_unit(_p(r, _f32p), _p(g, _f32p), _p(b, _f32p), W, H, reg, out_cols, out_rows, _p(con, _f32p),
                                        _p(out, _f32p), _c.byref(dev))
        assert rc == 0, "ffx_ref_easu_unit: %d" % rc
        return out, float(dev.value)


_cache = {}


def load(path=LIB):
    """The library, or a failure that says how to get it: it is built, never skipped."""
    if path not in _cache:
        if not os.path.exists(path):
            import pytest
            pytest.fail("%s is missing: build() makes it (`make -C oracle ref`, where the reference tree is present)" % os.path.relpath(path, ROOT))
        _cache[path] = FfxRef(path)
    return _cache[path]
