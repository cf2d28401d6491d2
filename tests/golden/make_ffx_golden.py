"""Generates tests/golden/ffx_ref.npz: results of the reference's own CAS and FSR shader text and host constants, from
oracle/_ref/libffx_ref.so (`make -C oracle ref`, where the reference tree is present), on a few small seeded inputs.  The file holds the
inputs and the recorded results only; tests/test_ffx_ref.py holds tests/np_cas.py and tests/np_fsr.py to it bit for bit, and checks that
the library still computes what the file holds.

    python tests/golden/make_ffx_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

f32 = np.float32
CAS_SHARPNESS = (0.3, 0.8)
EASU_CASES = (((0, 0, 65, 17), (33, 130)), ((0, 0, 65, 17), (7, 11)), ((3, 2, 61, 11), (33, 130)))   # (region, (out rows, out cols))
CON_CASES = ((1920, 1080, 1920, 1080, 3840, 2160), (1280, 720, 1280, 720, 1920, 1080), (3840, 2160, 3840, 2160, 1920, 1080),
             (1917, 1001, 1999, 1030, 3001, 777), (61, 11, 65, 17, 130, 33), (1, 1, 1, 1, 4096, 3))


def load_unit(img):
    return (np.asarray(img, np.float64) / 255.0).astype(f32)


def record(ref):
    rng = np.random.default_rng(0x46465831)
    d = {}
    img = rng.integers(0, 256, (17, 65, 3), dtype=np.uint8)
    img[:8, :30] = rng.integers(0, 256, 3, dtype=np.uint8)
    d["cas_img"] = img
    d["cas_sharpness"] = np.array(CAS_SHARPNESS, f32)
    d["cas_peak_bits"] = np.array([ref.cas_setup(s)[0] for s in CAS_SHARPNESS], np.uint32)
    for k, s in enumerate(CAS_SHARPNESS):
        d["cas_out_%d" % k] = ref.cas_unit(load_unit(img), ref.peak(s))[..., :3].copy()
    img = rng.integers(0, 256, (17, 65, 3), dtype=np.uint8)
    img[9:, 20:50, 1] = np.arange(30, dtype=np.uint8) * 8
    d["easu_img"] = img                                                                # B, G, R bytes
    d["easu_region"] = np.array([c[0] for c in EASU_CASES], np.int32)
    d["easu_out_size"] = np.array([c[1] for c in EASU_CASES], np.int32)
    x = load_unit(img)
    for k, (region, (oh, ow)) in enumerate(EASU_CASES):
        d["easu_out_%d" % k] = ref.easu_unit(x[..., 2], x[..., 1], x[..., 0], region, oh, ow)[0][..., :3].copy()
    d["con_cases"] = np.array(CON_CASES, np.int32)
    d["con_bits"] = np.stack([ref.easu_con(*c).view(np.uint32) for c in CON_CASES])
    return d


if __name__ == "__main__":
    from tests import ffx_ref_lib
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ffx_ref.npz")
    np.savez_compressed(out, **record(ffx_ref_lib.FfxRef(ffx_ref_lib.LIB)))
    print(out, os.path.getsize(out), "bytes")
