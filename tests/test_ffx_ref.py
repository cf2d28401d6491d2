"""The CAS and FSR specifications (tests/np_cas.py, tests/np_fsr.py) against the reference's own shader text: cas.effect, fsr.effect and
the FidelityFX headers they include, compiled for the host into oracle/_ref/libffx_ref.so by `make -C oracle ref` (tests/ffx_ref_lib.py),
and the host constants of np_* and of the C-ABI against the reference's CasSetup and FsrEasuCon.

Everything is equality of float32 bit patterns or of bytes; there is no tolerance.  What the reference leaves to the graphics API and
the compiled shim decides (oracle/ffx_ref/shim.h; DESIGN.md sections 14 and 16): a Load outside the frame reads 0, the point sampler
takes clamp(floor(u W), 0, W - 1), rcp is 1 / x, min / max drop a NaN operand.  What stays the specification's own: the u8 load
(u / 255, correctly rounded) and store (rint(255 v), half to even), and which bytes of a pixel are the shader's r, g, b; the test states
both again below, on the reference's side of each comparison.

The mutation tests change one reading of the shader text in np_* and require that the comparison then fails: the pin has teeth.  The
frozen tests hold np_* to tests/golden/ffx_ref.npz (recorded from the library by tests/golden/make_ffx_golden.py), for checkouts
that have neither the reference tree nor oracle/_ref/."""
import ctypes
import os

import numpy as np
import pytest

from tests import ffx_ref_lib
from tests import np_cas as nc
from tests import np_fsr as nf
from tests.test_cas_gpu import content
from tests.test_fsr_gpu import SMALL_IN, SMALL_OUT
from tests.test_fsr_spec import CON_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ffx_ref.npz")
f32 = np.float32
BGR, BGRA, RGB, RGBA, YUV = nf.FMT_BGR, nf.FMT_BGRA, nf.FMT_RGB, nf.FMT_RGBA, nf.FMT_YUV
FORMATS = [BGR, BGRA, RGB, RGBA, YUV]
# byte index of the shader's .r, .g, .b in a pixel of each format, stated here independently of np_fsr.channel_bytes (declared choice 3
# of DESIGN.md section 16: OBS hands the shader red, green, blue; a YUV frame goes through as bytes 0, 1, 2)
REF_RGB = {BGR: (2, 1, 0), BGRA: (2, 1, 0), RGB: (0, 1, 2), RGBA: (0, 1, 2), YUV: (0, 1, 2)}


@pytest.fixture(scope="module")
def ref():
    return ffx_ref_lib.load()


@pytest.fixture(scope="module")
def ref_f32lit():
    return ffx_ref_lib.load(ffx_ref_lib.LIB_F32LIT)


def _lib():
    from livevisionkit_amd import _native
    return _native.load()


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _word(v):
    return int(_bits(v).reshape(-1)[0])


def same_f32(got, want):
    """The NaN pattern first, then the values outside it, then every bit (which adds the sign of zero and the NaN payloads)."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return bool(np.array_equal(got[ok], want[ok])) and bool(np.array_equal(_bits(got), _bits(want)))


def load_unit(img):
    """The specification's load, restated: u / 255 in float64 (exact to well below half a float32 ulp) rounded once to float32."""
    return (np.asarray(img, np.float64) / 255.0).astype(f32)


def store_u8(v):
    """The specification's store, restated: 255 v in float32, round half to even."""
    return np.rint(np.asarray(v, f32) * f32(255)).astype(np.uint8)


# ---- CAS ------------------------------------------------------------------------------------------------------------------------------

CAS_SIZES = [(1, 1), (1, 2), (2, 1), (3, 5), (17, 65), (270, 480)]
CAS_SHARPNESS = [0.0, 0.3, 0.8, 1.0, -0.5, 1.5, 7.0]


def every_byte_frame(ch=3):
    """tests/test_cas_gpu.py's frame: each of the nine positions around an interior centre sees every byte value."""
    y, x = np.mgrid[0:258, 0:258]
    return np.stack([(x + 7 * y + 85 * c) % 256 if c % 2 == 0 else (y + 7 * x + 85 * c) % 256 for c in range(ch)], -1).astype(np.uint8)


def cas_frames(rows, cols, ch=3):
    rng = np.random.default_rng(rows * 1000 + cols)
    yield "random", rng.integers(0, 256, (rows, cols, ch), dtype=np.uint8)
    yield "patches", content(rows, cols, ch, seed=rows + cols)
    blocks = rng.integers(0, 256, ((rows + 7) // 8, (cols + 7) // 8, ch), dtype=np.uint8)
    yield "blocky", np.repeat(np.repeat(blocks, 8, 0), 8, 1)[:rows, :cols]
    for v in (0, 1, 127, 200, 255):
        yield "flat%d" % v, np.full((rows, cols, ch), v, np.uint8)
    # windows with mx = 0 (all nine zero) next to windows with mn = 0 and mx > 0: lone bright pixels on black, lone black ones on white
    sparse = np.zeros((rows, cols, ch), np.uint8)
    sparse[::5, ::7] = rng.integers(1, 256, sparse[::5, ::7].shape, dtype=np.uint8)
    yield "sparse", sparse
    holes = rng.integers(200, 256, (rows, cols, ch), dtype=np.uint8)
    holes[1::4, 2::3] = 0
    yield "holes", holes


def ref_cas_bytes(ref, img, sharpness):
    """The reference's CasSetup and pixel shader between the specification's load and store; the shader's 4th component is stored too."""
    y = ref.cas_unit(load_unit(img[..., :3]), ref.peak(sharpness))
    return store_u8(y)[..., :img.shape[2]]


@pytest.mark.parametrize("rows,cols", CAS_SIZES)
def test_cas_is_the_reference_shader(ref, rows, cols):
    for name, img in cas_frames(rows, cols):
        x = nc.UNIT[img]
        assert np.array_equal(_bits(x), _bits(load_unit(img)))
        for s in CAS_SHARPNESS:
            got = nc.cas_unit(x, nc.peak_of(s))
            want = ref.cas_unit(x, ref.peak(s))
            assert same_f32(want[..., 3], np.ones((rows, cols), f32)), (name, s)
            assert same_f32(got, want[..., :3]), (name, s, int((_bits(got) != _bits(want[..., :3])).sum()))
            assert np.array_equal(nc.cas(img, s), ref_cas_bytes(ref, img, s)), (name, s)


def test_cas_every_byte_value_in_every_neighbour_position(ref):
    img = every_byte_frame()
    x = nc.UNIT[img]
    for s in (0.0, 0.3, 0.8, 1.0):
        assert same_f32(nc.cas_unit(x, nc.peak_of(s)), ref.cas_unit(x, ref.peak(s))[..., :3]), s
        assert np.array_equal(nc.cas(img, s), ref_cas_bytes(ref, img, s)), s


def test_cas_fourth_channel_is_the_shaders_one(ref):
    img = content(17, 65, 4, seed=4)
    img[..., 3] = np.arange(65, dtype=np.uint8)
    assert np.array_equal(nc.cas(img, 0.8), ref_cas_bytes(ref, img, 0.8))


CAS_OUT_OF_RANGE = [-1.0, -0.0, -1e-30, 1.0000001, 2.0, 1e30, -1e30, float("inf"), float("-inf")]


def test_cas_constant_is_cas_setup(ref):
    """np_cas.peak_of and lvk_hip_cas_const against const1.x of CasSetup over 2^16 sharpness values on [0, 1] and values outside it.
    CASEffect::configure passes the sharpness on as it is (it only asserts the range in debug builds); the clamp is CasSetup's own ASatF1,
    so the out-of-range values go to all three unclamped.  A NaN is refused by the library; CasSetup is not asked."""
    lib = _lib()
    grid = np.linspace(0.0, 1.0, 1 << 16).astype(f32)
    assert grid[0] == 0 and grid[-1] == 1 and len(np.unique(grid)) == 1 << 16
    peak = ctypes.c_float()
    for s in list(grid) + [f32(v) for v in CAS_OUT_OF_RANGE]:
        words = ref.cas_setup(s)
        want = int(words[0])
        assert _word(nc.peak_of(s)) == want, float(s)
        assert lib.lvk_hip_cas_const(ctypes.c_float(s), ctypes.byref(peak)) == 0
        assert _word(peak.value) == want, float(s)
        assert int(words[3]) == 0


# ---- FSR ------------------------------------------------------------------------------------------------------------------------------

def ref_fsr_unit(ref, img, fmt, region, oh, ow):
    """The reference's FsrEasuCon and EASU pixel shader behind the specification's load, with the byte mapping of REF_RGB: the shader's
    float4 per pixel and the largest distance of a sampled coordinate from a texel centre."""
    x = load_unit(img)
    ri, gi, bi = REF_RGB[fmt]
    return ref.easu_unit(x[..., ri], x[..., gi], x[..., bi], region, oh, ow)


def ref_fsr_store(y, fmt, ch):
    """The specification's store of the shader's float4 (r, g, b, a) into pixels of the format; the shader's 4th component is stored too."""
    q = store_u8(y)
    ri, gi, bi = REF_RGB[fmt]
    out = np.empty(y.shape[:2] + (ch,), np.uint8)
    out[..., ri], out[..., gi], out[..., bi] = q[..., 0], q[..., 1], q[..., 2]
    if ch == 4:
        out[..., 3] = q[..., 3]
    return out


def check_fsr(ref, img, fmt, region, oh, ow):
    x = nc.UNIT[img]
    assert np.array_equal(_bits(x), _bits(load_unit(img)))
    ri, gi, bi = REF_RGB[fmt]
    want, dev = ref_fsr_unit(ref, img, fmt, region, oh, ow)
    # the invariant behind declared choice 6, on the coordinates the reference's own gather functions computed
    assert dev < 0.25, dev
    assert same_f32(want[..., 3], np.ones((oh, ow), f32))
    got = nf.easu_unit(x[..., ri], x[..., gi], x[..., bi], region, oh, ow)
    assert same_f32(got, want[..., :3]), "%d of %d values differ" % (int((_bits(got) != _bits(want[..., :3])).sum()), got.size)
    assert np.array_equal(nf.fsr(img, fmt, region, oh, ow), ref_fsr_store(want, fmt, img.shape[2]))


CROPS = [(0, 0, 20, 15), (37, 0, 20, 15), (0, 25, 20, 15), (37, 25, 20, 15), (1, 1, 55, 38), (56, 39, 1, 1), (0, 0, 57, 1)]


def small_corpus():
    """(img, fmt, region, oh, ow) of the small cases: tests/test_fsr_gpu.py's sizes, crops, formats and the two kernel paths' shapes."""
    for rows, cols in SMALL_IN:
        img = content(rows, cols, 3, seed=rows * 100 + cols)
        for oh, ow in SMALL_OUT:
            yield img, BGR, (0, 0, cols, rows), oh, ow
    for region in CROPS:
        img = content(40, 57, 4, seed=sum(region))
        for oh, ow in ((region[3] * 2, region[2] * 2), (31, 17), (1, 1)):
            yield img, RGBA, region, oh, ow
    for fmt in FORMATS:
        img = content(45, 77, nf.CHANNELS[fmt], seed=fmt)
        for oh, ow in ((90, 154), (30, 50), (45, 200)):
            yield img, fmt, (0, 0, 77, 45), oh, ow


@pytest.mark.parametrize("rows,cols", SMALL_IN)
def test_fsr_small_inputs_at_many_output_sizes(ref, rows, cols):
    img = content(rows, cols, 3, seed=rows * 100 + cols)
    for oh, ow in SMALL_OUT:
        check_fsr(ref, img, BGR, (0, 0, cols, rows), oh, ow)


@pytest.mark.parametrize("region", CROPS)
def test_fsr_crops_touching_each_frame_edge(ref, region):
    img = content(40, 57, 4, seed=sum(region))
    for oh, ow in ((region[3] * 2, region[2] * 2), (31, 17), (1, 1)):
        check_fsr(ref, img, RGBA, region, oh, ow)


@pytest.mark.parametrize("fmt", FORMATS)
def test_fsr_every_format(ref, fmt):
    img = content(45, 77, nf.CHANNELS[fmt], seed=fmt)
    for oh, ow in ((90, 154), (30, 50), (45, 200)):
        check_fsr(ref, img, fmt, (0, 0, 77, 45), oh, ow)


STAGED_CASES = [(300, 500, (0, 0, 500, 300), 700, 1100), (300, 500, (3, 5, 400, 250), 250, 400), (300, 500, (0, 0, 500, 300), 1, 1)]
DIRECT_CASES = [(300, 500, (0, 0, 500, 300), 150, 250), (300, 500, (0, 0, 500, 300), 30, 400), (300, 500, (7, 2, 480, 290), 290, 100),
                (300, 500, (0, 0, 500, 300), 200, 333), (300, 500, (0, 0, 500, 300), 5, 7)]


@pytest.mark.parametrize("rows,cols,region,oh,ow", STAGED_CASES)
def test_fsr_shapes_of_the_staged_path(ref, rows, cols, region, oh, ow):
    assert _lib().lvk_hip_fsr_easu_path(region[2], region[3], oh, ow) == 0
    check_fsr(ref, content(rows, cols, 3, seed=oh), YUV, region, oh, ow)


@pytest.mark.parametrize("rows,cols,region,oh,ow", DIRECT_CASES)
def test_fsr_shapes_of_the_direct_path(ref, rows, cols, region, oh, ow):
    assert _lib().lvk_hip_fsr_easu_path(region[2], region[3], oh, ow) == 1
    check_fsr(ref, content(rows, cols, 4, seed=oh), BGRA, region, oh, ow)


@pytest.mark.parametrize("rows,cols,region,oh,ow,fmt,textured", [
    (720, 1280, (0, 0, 1280, 720), 1080, 1920, BGR, False),             # con0.x != con0.y (tests/test_fsr_spec.py's second case)
    (1080, 1920, (0, 0, 1920, 1080), 2160, 3840, BGRA, True),
    (2160, 3840, (0, 0, 3840, 2160), 1080, 1920, BGR, True),
    (1030, 1999, (41, 17, 1917, 1001), 777, 3001, RGBA, False),
])
def test_fsr_frame_sizes(ref, rows, cols, region, oh, ow, fmt, textured):
    from tests import synth
    ch = nf.CHANNELS[fmt]
    if textured:
        img = synth.textured_frame(rows, cols, seed=rows + cols)
        if ch == 4:
            img = np.concatenate([img, np.full((rows, cols, 1), 9, np.uint8)], -1)
    else:
        img = content(rows, cols, ch, seed=rows + cols)
    if (rows, cols, oh, ow) == (720, 1280, 1080, 1920):
        c = ref.easu_con(cols, rows, cols, rows, ow, oh)
        assert c[0] != c[1]
    check_fsr(ref, img, fmt, region, oh, ow)


def con_cases():
    rng = np.random.default_rng(0xEA5C)
    yield from sorted(CON_CASES)
    yield from [(1917, 1001, 1999, 1030, 3001, 777), (7, 5, 13, 11, 1, 1), (1, 1, 1, 1, 4096, 3), (1900, 1080, 1920, 1080, 3800, 2160),
                (640, 360, 1920, 1080, 1920, 1080), (3, 4097, 5, 4099, 4096, 4096)]
    for _ in range(3000):
        W, H, ow, oh = (int(v) for v in rng.integers(1, 4097, 4))
        yield int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1)), W, H, ow, oh


def test_fsr_constants_are_fsr_easu_con(ref):
    lib = _lib()
    con = (ctypes.c_float * 16)()
    n = 0
    for case in con_cases():
        want = _bits(ref.easu_con(*case))
        assert np.array_equal(_bits(nf.easu_const(*case)), want), case
        assert lib.lvk_hip_fsr_easu_const(*case, con) == 0, case
        assert np.array_equal(_bits(list(con)), want), case
        n += 1
    assert n == 3009
    for case in sorted(CON_CASES):
        assert [int(b) for b in _bits(ref.easu_con(*case))] == CON_CASES[case]


# ---- the pixel position, and the typing of the literals --------------------------------------------------------------------------------

def test_pixel_centre_uv_gives_the_integer_pixel_back():
    """The shaders take pos = floor(uv * output_size) of an interpolated uv; the specification takes the integer x.  For the one model of
    the interpolation that can be stated, uv = f32((x + 0.5) / ow), the two are the same for every ow <= 4096 and every x < ow (the
    compiled driver uses that model and checks the same per pixel)."""
    bad = []
    for ow in range(1, nf.MAX_DIMENSION + 1):
        x = np.arange(ow, dtype=f32)
        uv = (x + f32(0.5)) / f32(ow)
        assert uv.dtype == f32
        pos = np.floor(uv * f32(ow))
        bad += [(int(i), ow) for i in np.nonzero(pos != x)[0]]
    assert bad == []


def test_literal_typing_does_not_matter(ref, ref_f32lit):
    """HLSL types 2.0/5.0, 25.0/16.0 and (1.0/4.0-0.04)-0.5 as float expressions; C++ folds them in double and rounds once (np_fsr's
    reading).  The library built with every literal typed as float computes the same bits over the small corpus and the CAS frames, and the
    constants have the same bit patterns either way."""
    one = lambda v: f32(v)                                                               # noqa: E731
    assert _word(one(2.0) / one(5.0)) == _word(nf.W_B)
    assert _word(one(25.0) / one(16.0)) == _word(nf.W_SCALE)
    assert _word(-(one(25.0) / one(16.0) - one(1.0))) == _word(nf.W_BIAS)
    assert _word((one(1.0) / one(4.0) - one(0.04)) - one(0.5)) == _word(nf.LOB_SLOPE)
    assert _word(one(1.0) / one(32768.0)) == _word(nf.DIR_EPS)
    for img, fmt, region, oh, ow in small_corpus():
        x = nc.UNIT[img]
        ri, gi, bi = REF_RGB[fmt]
        a, _ = ref.easu_unit(x[..., ri], x[..., gi], x[..., bi], region, oh, ow)
        b, _ = ref_f32lit.easu_unit(x[..., ri], x[..., gi], x[..., bi], region, oh, ow)
        assert same_f32(a, b)
    for rows, cols in CAS_SIZES[:5]:
        for _, img in cas_frames(rows, cols):
            x = nc.UNIT[img]
            assert same_f32(ref.cas_unit(x, ref.peak(0.8)), ref_f32lit.cas_unit(x, ref_f32lit.peak(0.8)))


# ---- the pin has teeth: one misreading of the shader text each, and the comparison must fail ----------------------------------------

def fsr_matches(ref):
    for img, fmt, region, oh, ow in small_corpus():
        x = nc.UNIT[img]
        ri, gi, bi = REF_RGB[fmt]
        want, _ = ref.easu_unit(x[..., ri], x[..., gi], x[..., bi], region, oh, ow)
        if not same_f32(nf.easu_unit(x[..., ri], x[..., gi], x[..., bi], region, oh, ow), want[..., :3]):
            return False
    return True


def cas_matches(ref):
    for rows, cols in CAS_SIZES[:5]:
        for _, img in cas_frames(rows, cols):
            x = nc.UNIT[img]
            for s in (0.0, 0.8):
                if not same_f32(nc.cas_unit(x, nc.peak_of(s)), ref.cas_unit(x, ref.peak(s))[..., :3]):
                    return False
    return True


def test_mutation_corpus_matches_unmutated(ref):
    assert fsr_matches(ref) and cas_matches(ref)


def test_mutation_lob_slope_in_float32_steps_is_the_same_constant(ref, monkeypatch):
    """(1.0/4.0-0.04)-0.5 taken in float32 steps has the bit pattern of the double expression rounded once, so this reading cannot be told
    from the specification's by any test (test_literal_typing_does_not_matter).  The constant itself is pinned: one ulp either way fails."""
    steps = (f32(1.0) / f32(4.0) - f32(0.04)) - f32(0.5)
    assert _word(steps) == _word(nf.LOB_SLOPE)
    for toward in (f32(-1), f32(0)):
        monkeypatch.setattr(nf, "LOB_SLOPE", np.nextafter(steps, toward))
        assert not fsr_matches(ref)


def test_mutation_two_taps_of_the_order_swapped(ref, monkeypatch):
    monkeypatch.setattr(nf, "ORDER", "bcijefklhgon")
    assert not fsr_matches(ref)


def test_mutation_luma_in_another_association(ref, monkeypatch):
    monkeypatch.setattr(nf, "luma", lambda tr, tg, tb: (tb * f32(0.5) + tr * f32(0.5)) + tg)
    assert not fsr_matches(ref)


def test_mutation_second_gather_with_x_and_y_exchanged(ref, monkeypatch):
    gathers = list(nf.GATHERS)
    gathers[1] = ("j", "i", "f", "e")
    monkeypatch.setattr(nf, "GATHERS", gathers)
    assert not fsr_matches(ref)


def test_mutation_lo_rcp_with_med_rcps_constant(ref, monkeypatch):
    monkeypatch.setattr(nc, "LO_RCP_BITS", nc.MED_RCP_BITS)
    assert not fsr_matches(ref)
    assert not cas_matches(ref)


def test_mutation_cas_soft_min_without_the_diagonal_term(ref, monkeypatch):
    def plus_only(a, b, c, d, e, f, g, h, i):
        mn = np.minimum(np.minimum(np.minimum(d, e), f), np.minimum(b, h))
        return mn + mn
    monkeypatch.setattr(nc, "soft_min", plus_only)
    assert not cas_matches(ref)


def test_mutation_cas_sum_in_another_association(ref, monkeypatch):
    monkeypatch.setattr(nc, "weighted_sum", lambda b, d, f, h, e, w: ((b * w + d * w) + (f * w + h * w)) + e)
    assert not cas_matches(ref)


# ---- the frozen copy --------------------------------------------------------------------------------------------------------------------

def test_frozen_reference_results():
    """np_cas / np_fsr against results recorded from the library (tests/golden/make_ffx_golden.py): needs neither oracle/_ref/ nor the
    reference tree."""
    z = np.load(GOLDEN)
    img = z["cas_img"]
    for k, s in enumerate(z["cas_sharpness"]):
        assert _word(nc.peak_of(s)) == int(z["cas_peak_bits"][k])
        assert same_f32(nc.cas_unit(nc.UNIT[img], nc.peak_of(s)), z["cas_out_%d" % k])
    img = z["easu_img"]
    x = nc.UNIT[img]
    for k in range(len(z["easu_region"])):
        region = tuple(int(v) for v in z["easu_region"][k])
        oh, ow = (int(v) for v in z["easu_out_size"][k])
        assert same_f32(nf.easu_unit(x[..., 2], x[..., 1], x[..., 0], region, oh, ow), z["easu_out_%d" % k])
    for k, case in enumerate(z["con_cases"]):
        assert np.array_equal(_bits(nf.easu_const(*(int(v) for v in case))), z["con_bits"][k])


def test_frozen_file_is_what_the_library_computes(ref):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ffx_golden", os.path.join(ROOT, "tests", "golden", "make_ffx_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    fresh = maker.record(ref)
    z = np.load(GOLDEN)
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        assert z[k].dtype == fresh[k].dtype and z[k].shape == fresh[k].shape and z[k].tobytes() == fresh[k].tobytes(), k


def test_frozen_file_is_small():
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_kernels.npz"))
