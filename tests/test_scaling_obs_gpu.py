"""lvk_hip_scale_obs on the MI355X (csrc/scaling_obs.hip): the planes of every OBS video format, out of place, bit for bit against
the specification of tests/scaling_obs_cases.py (oracle ingest_obs -> upscale -> sharpen -> egress_obs; its liveness: tests/test_scaling_obs_spec.py) and
against the GPU's own four-call chain.  Every plane is a view into a buffer of guard bytes (the helpers of tests/test_lens_obs_gpu.py): pitch padding,
what lies before and behind a plane, and the bytes lvk_hip_egress_obs leaves alone (the last quarter of an RGBA / BGRA / BGRX plane) must come back
unchanged, and so must the input planes."""
import ctypes

import numpy as np
import pytest

from tests.scaling_obs_cases import (ALL_CASES, DIRECT4, F420, F422, FORMATS, FRAME_YUV, GUARD, SIZES_420, SIZES_422, SIZES_444, case_id, expected,
                                     oracle, sizes_of, textures_of)
from tests.test_lens_obs_gpu import Buf, arr3, assert_outputs, gpu, guarded_outputs, raw_fn, written

pytestmark = pytest.mark.gpu

ERR_ARG = -1
_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
SIGNATURE = [_P, _I, _P, _P, _I, _I, _P, _P, _I, _I, _F]


def placement(fmt, pads, offsets):
    """The 4-byte DirectIngest planes are tight (steps[0] == 4 * cols); every other plane, AYUV included, takes any pitch and any first byte."""
    return ((0, 0, 0), offsets) if fmt in DIRECT4 else (pads, offsets)


def scale_guarded(ctx, case, kind, pads=(0, 0, 0), offsets=(0, 0, 0), what=""):
    fmt, src, dst, sharpness = case
    e = expected(case, kind)
    pads, offsets = placement(fmt, pads, offsets)
    ins = [Buf(p, pads[i], offsets[i], seed=10 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], pads, offsets)
    views = [p.view for p in outs]
    got = ctx.scale_obs(fmt, [p.view for p in ins], size=(dst[1], dst[0]), sharpness=sharpness, out=views)
    assert all(g is v for g, v in zip(got, views))
    ctx.sync()
    for i, p in enumerate(ins):
        assert p.unchanged(), "%s %s: input plane %d changed" % (what, kind, i)
    assert_outputs(outs, e["want"], "%s %s" % (what, kind))


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_scale_obs_bit_exact(ctx, case):
    """Through the C-ABI into padded, offset planes of guard bytes: tight planes for the first texture, pitches + 1 / + 13 and bases 1 .. 3 bytes off a
    dword for the second."""
    for k, kind in enumerate(textures_of(case)):
        scale_guarded(ctx, case, kind, pads=(k, 13 * k, k), offsets=(k, k, 3 * k), what=case_id(case))


def three_of(fmt):
    s = sizes_of(fmt)
    return [s[2], s[3], s[4]] if fmt in F420 else [s[5], s[7], s[-1]]


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_call_equals_the_four_call_chain_on_the_device(ctx, fmt):
    import torch
    for src, dst in three_of(fmt):
        e = expected((fmt, src, dst, 0.8), "smooth")
        planes = [gpu(p) for p in e["planes"]]
        size = (dst[1], dst[0])
        one = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
        chained = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
        ctx.scale_obs(fmt, planes, size=size, sharpness=0.8, out=one)
        frame = ctx.ingest_obs(fmt, planes)
        if fmt == "Y800":
            sharpened = ctx.sharpen_gray(ctx.upscale_gray(frame, size), 0.8)
        else:
            sharpened = ctx.sharpen(ctx.upscale(frame, size, yuv=fmt in FRAME_YUV), 0.8)
        ctx.egress_obs(fmt, sharpened, chained)
        ctx.sync()
        for i, (a, b, w) in enumerate(zip(one, chained, e["want"])):
            assert torch.equal(a, b), (fmt, src, dst, i)
            assert np.array_equal(a.cpu().numpy(), w), (fmt, src, dst, i)


@pytest.mark.parametrize("pair", [SIZES_444[5], SIZES_444[6], SIZES_444[9], SIZES_444[11]], ids=lambda p: "%dx%d-%dx%d" % (*p[0], *p[1]))
def test_ayuv_planes_based_at_an_odd_byte(ctx, pair):
    """Both fused routes: the plane source loads and the sink stores dwords only where the address allows."""
    for off, pad in ((1, 0), (3, 1), (2, 2), (1, 7)):
        scale_guarded(ctx, ("AYUV", *pair, 0.8), "random", pads=(pad, 0, 0), offsets=(off, 0, 0), what="AYUV +%d pad %d" % (off, pad))


@pytest.mark.parametrize("equal", [False, True], ids=["upscale", "equal"])
@pytest.mark.parametrize("fmt", ["I422", "YUY2", "I444", "AYUV", "BGR3", "RGBA", "Y800", "I420", "NV12"])
def test_refused_calls_change_nothing(ctx, fmt, equal):
    src = (16, 34)
    dst = src if equal else (22, 42)
    rows, cols = src
    drows, dcols = dst
    vf = ctx.VIDEO_FORMATS[fmt]
    case = (fmt, src, dst, 0.8)
    e = expected(case, "random")
    pad = 0 if fmt in DIRECT4 else 4
    ins = [Buf(p, pad, 0, seed=20 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], (pad,) * 3)
    n = len(ins)
    ip, isteps = [p.view.data_ptr() for p in ins], [p.pitch for p in ins]
    op, osteps = [p.view.data_ptr() for p in outs], [p.pitch for p in outs]
    irow, orow = [p.row for p in ins], [p.row for p in outs]
    prows = [p.shape[0] for p in ins]
    fn = raw_fn(ctx, "lvk_hip_scale_obs", SIGNATURE)

    def call(handle=ctx.handle, vf=vf, ip=ip, isteps=isteps, op=op, osteps=osteps, src=src, dst=dst, sharpness=0.8, null=()):
        a = [None if "ip" in null else arr3(ip, _P), None if "isteps" in null else arr3(isteps, _I),
             None if "op" in null else arr3(op, _P), None if "osteps" in null else arr3(osteps, _I)]
        return fn(handle, vf, a[0], a[1], src[0], src[1], a[2], a[3], dst[0], dst[1], sharpness)

    def unchanged():
        ctx.sync()
        return all(p.unchanged() for p in outs) and all(p.unchanged() for p in ins)

    refused = [dict(handle=None), dict(null=("ip",)), dict(null=("isteps",)), dict(null=("op",)), dict(null=("osteps",))]
    refused += [dict(vf=v) for v in (0, 17, -1, 99)]                                # an unknown format
    refused += [dict(src=s) for s in [(0, cols), (rows, 0), (-2, cols), (rows, -2)]]
    refused += [dict(dst=s) for s in [(0, dcols), (drows, 0), (-2, dcols), (rows - 2, dcols), (drows, cols - 2)]]      # Image.cpp:157: no smaller
    refused += [dict(sharpness=s) for s in (-0.01, 1.01, float("nan"), float("inf"), -float("inf"))]
    if fmt in F422 or fmt in F420:
        refused += [dict(src=(rows, cols - 1)), dict(dst=(drows, dcols + 1)), dict(dst=(drows, dcols - 1) if not equal else (drows, dcols + 3))]    # odd cols
    if fmt in F420:
        refused += [dict(src=(rows - 1, cols)), dict(dst=(drows + 1, dcols))]       # odd rows
    for i in range(n):
        refused.append(dict(ip=ip[:i] + [None] + ip[i + 1:]))                       # a NULL plane that is in use
        refused.append(dict(op=op[:i] + [None] + op[i + 1:]))
        refused.append(dict(isteps=isteps[:i] + [irow[i] - 1] + isteps[i + 1:]))    # a pitch below its row
        refused.append(dict(osteps=osteps[:i] + [orow[i] - 1] + osteps[i + 1:]))
        if fmt not in F420:                                                         # a plane the kernels' 32-bit offsets cannot address
            refused.append(dict(osteps=osteps[:i] + [1 << 24] + osteps[i + 1:]))
            refused.append(dict(isteps=isteps[:i] + [1 << 24] + isteps[i + 1:]))
        refused.append(dict(op=op[:i] + [ip[0]] + op[i + 1:]))                      # in place, and ending inside an input plane
        refused.append(dict(op=op[:i] + [ip[n - 1] + isteps[n - 1] * (prows[n - 1] - 1) + irow[n - 1] - 1] + op[i + 1:]))
    if fmt in DIRECT4:
        refused += [dict(isteps=[4 * cols + 4]), dict(osteps=[4 * dcols + 4]), dict(isteps=[4 * cols - 4]), dict(osteps=[4 * dcols - 4])]
    if n == 3:
        refused.append(dict(op=[op[0], op[0] + osteps[0] * (drows - 1), op[2]]))    # two outputs on each other
        refused.append(dict(op=[op[0], op[1], op[1] + 1]))
    if n == 2:
        refused.append(dict(op=[op[0], op[0] + osteps[0] * (drows - 1)]))
    for a in refused:
        assert call(**a) == ERR_ARG, a
        assert "handle" in a or ctx.lib.lvk_hip_last_error(ctx.handle), a                # every refusal of a live context leaves its message
        assert unchanged(), a
    assert call() == 0
    ctx.sync()
    assert_outputs(outs, e["want"], "after the refusals")
    assert all(p.unchanged() for p in ins)


@pytest.mark.parametrize("fmt", ["UYVY", "I444", "BGR3", "Y800"])
def test_steady_state_allocates_nothing(ctx, fmt):
    """As tests/test_lens_obs_gpu.py taps it: the pool is emptied and given ONE block of each size the route needs, filled with a pattern.  Every call must
    take those blocks and give them back: afterwards lvk_hip_malloc of the sizes hands out the same addresses, and the blocks hold the frames the call made
    in them (the ingested and the upscaled frame) -- a call that allocated memory of its own would leave the pattern, one that kept a block would make
    lvk_hip_malloc hand out another.  Three calls in a row."""
    src, dst = (135, 240), (270, 480)
    case = (fmt, src, dst, 0.8)
    e = expected(case, "smooth")
    fused = fmt in ("UYVY", "I444")
    bpp = 1 if fmt == "Y800" else 3
    held_want = ([np.ascontiguousarray(e["packed"])] if fused else []) + [np.ascontiguousarray(e["scaled"])]
    sizes = [((bpp * s[1] + 3) & ~3) * s[0] for s in (([src] if fused else []) + [dst])]
    assert sizes == [w.size for w in held_want]
    planes = [gpu(p) for p in e["planes"]]
    L = ctx.lib
    ctx.sync()
    assert L.lvk_hip_trim(ctx.handle) == 0
    blocks = [ctypes.c_void_p() for _ in sizes]
    for b, nbytes in zip(blocks, sizes):
        assert L.lvk_hip_malloc(ctx.handle, nbytes, ctypes.byref(b)) == 0
    for _ in range(3):
        for b, nbytes in zip(blocks, sizes):
            pattern = np.full(nbytes, GUARD, np.uint8)
            assert L.lvk_hip_upload(ctx.handle, b, pattern.ctypes.data_as(ctypes.c_void_p), nbytes) == 0
        ctx.sync()
        for b in blocks:
            assert L.lvk_hip_free(ctx.handle, b) == 0
        got = ctx.scale_obs(fmt, planes, size=(dst[1], dst[0]), sharpness=0.8)
        ctx.sync()
        for b, nbytes, want in zip(blocks, sizes, held_want):
            again = ctypes.c_void_p()
            assert L.lvk_hip_malloc(ctx.handle, nbytes, ctypes.byref(again)) == 0
            assert again.value == b.value
            held = np.zeros(nbytes, np.uint8)
            assert L.lvk_hip_download(ctx.handle, held.ctypes.data_as(ctypes.c_void_p), again, nbytes) == 0
            ctx.sync()
            assert np.array_equal(held.reshape(want.shape), want)
        assert written(fmt, [g.cpu().numpy() for g in got], e["want"])
    for b in blocks:
        assert L.lvk_hip_free(ctx.handle, b) == 0
    # equal sizes on the fused formats: one launch on the planes, nothing taken from the pool -- an empty pool stays empty of blocks to hand out
    if fused:
        assert L.lvk_hip_trim(ctx.handle) == 0
        eq = expected((fmt, src, src, 0.8), "smooth")
        got = ctx.scale_obs(fmt, planes, sharpness=0.8)
        ctx.sync()
        assert written(fmt, [g.cpu().numpy() for g in got], eq["want"])
        fresh = ctypes.c_void_p()
        assert L.lvk_hip_malloc(ctx.handle, sizes[0], ctypes.byref(fresh)) == 0    # (a block the call had pooled would come back here, filled)
        L.lvk_hip_upload(ctx.handle, fresh, np.full(sizes[0], GUARD, np.uint8).ctypes.data_as(ctypes.c_void_p), sizes[0])
        ctx.sync()
        assert L.lvk_hip_free(ctx.handle, fresh) == 0
    del planes


def test_alternating_formats_and_sizes_call_after_call(ctx):
    steps = 0
    for _ in range(2):
        for fmt, pair in [("UYVY", SIZES_422[-1]), ("I444", SIZES_444[5]), ("RGBA", SIZES_444[-2]), ("I420", SIZES_420[3]), ("Y800", SIZES_444[3]),
                          ("AYUV", SIZES_444[8]), ("BGR3", SIZES_444[-1]), ("I42A", SIZES_422[6]), ("NV12", SIZES_420[4]), ("YVYU", SIZES_422[5]),
                          ("YUVA", SIZES_444[-2]), ("I444", SIZES_444[11]), ("UYVY", SIZES_422[9])]:
            e = expected((fmt, *pair, 0.8), "smooth")
            got = ctx.scale_obs(fmt, [gpu(p) for p in e["planes"]], size=(pair[1][1], pair[1][0]))
            ctx.sync()
            assert written(fmt, [g.cpu().numpy() for g in got], e["want"]), (fmt, pair)
            steps += 1
    assert steps == 26


def test_the_python_methods_forms(ctx):
    import torch
    import livevisionkit_amd as lvk
    for fmt, pair in (("UYVY", SIZES_422[5]), ("I422", SIZES_422[6]), ("Y800", SIZES_444[5]), ("NV12", SIZES_420[2]), ("BGRA", SIZES_444[3])):
        src, dst = pair
        e = expected((fmt, src, dst, 0.8), "smooth")
        planes = [gpu(p) for p in e["planes"]]
        size = (dst[1], dst[0])
        by_name, by_number = ctx.scale_obs(fmt, planes, size=size), ctx.scale_obs(ctx.VIDEO_FORMATS[fmt], planes, size=size, sharpness=0.8)
        given = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
        back = ctx.scale_obs(fmt, tuple(planes), size=size, out=given)
        ctx.sync()
        assert isinstance(by_name, list) and all(b is g for b, g in zip(back, given))
        assert [tuple(a.shape) for a in by_name] == [w.shape for w in e["want"]]
        assert written(fmt, [a.cpu().numpy() for a in by_name], e["want"]) and written(fmt, [a.cpu().numpy() for a in by_number], e["want"])
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(given, e["want"]))
        with pytest.raises(ValueError):
            ctx.scale_obs(fmt, planes, size=size, out=given[:-1] if len(given) > 1 else given + given)
        with pytest.raises(lvk.LvkHipError):
            ctx.scale_obs(fmt, planes, size=size, sharpness=1.5)
        with pytest.raises(lvk.LvkHipError):
            ctx.scale_obs(fmt, planes, size=(src[1] - 2, src[0]))
    # size=None: the input's, sharpen only
    e = expected(("I444", *SIZES_444[6], 0.8), "smooth")
    got = ctx.scale_obs("I444", [gpu(p) for p in e["planes"]])
    ctx.sync()
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, e["want"]))
