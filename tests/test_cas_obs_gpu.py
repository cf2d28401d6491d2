"""lvk_hip_cas_yuv420 / lvk_hip_cas_obs on the MI355X (csrc/cas_420.hip, csrc/cas_obs.hip): the planes of every OBS video format,
out of place, bit for bit against the specification of tests/cas_obs_cases.py (oracle ingest_obs -> tests/np_cas.py -> egress_obs; its liveness:
tests/test_cas_obs_spec.py) and against the GPU's own three-call chain.  Every plane is a view into a buffer of guard bytes (the helpers of
tests/test_lens_obs_gpu.py): pitch padding, what lies before and behind a plane, and the bytes lvk_hip_egress_obs leaves alone (the last quarter of an
RGBA / BGRA / BGRX plane) must come back unchanged, and so must the input planes."""
import ctypes

import numpy as np
import pytest

from tests.cas_obs_cases import (CASES, DIRECT4, F420, F422, FORMATS, FULL, FULL_CASES, GUARD, SHARPNESS, case_id, expected, sharpness_of, sizes_of)
from tests.test_lens_obs_gpu import Buf, arr3, assert_outputs, gpu, guarded_outputs, raw_fn, written

pytestmark = pytest.mark.gpu

ERR_ARG = -1
FORMAT_BGR, FORMAT_RGB, FORMAT_YUV = 0, 2, 4
_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
SIGNATURE = [_P, _I, _P, _P, _P, _P, _I, _I, _F]
C_MID = (17, 34)                                       # a size every format outside 4:2:0 takes
C_MID_420 = (18, 34)


def mid(fmt):
    return C_MID_420 if fmt in F420 else C_MID


def placement(fmt, pads, offsets):
    """The 4-byte DirectIngest planes are tight (steps[0] == 4 * cols); every other plane, AYUV included, takes any pitch and any first byte."""
    return ((0, 0, 0), offsets) if fmt in DIRECT4 else (pads, offsets)


def new_filter(ctx, sharpness):
    import livevisionkit_amd as lvk
    return lvk.CASFilter(ctx, sharpness)


def frame_format(fmt):
    return FORMAT_RGB if fmt == "RGBA" else FORMAT_BGR if fmt in DIRECT4 + ["BGR3"] else FORMAT_YUV


def apply_guarded(ctx, f, fmt, size, pads=(0, 0, 0), offsets=(0, 0, 0), what=""):
    e = expected(fmt, size, f.sharpness)
    pads, offsets = placement(fmt, pads, offsets)
    ins = [Buf(p, pads[i], offsets[i], seed=10 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], pads[::-1], offsets[::-1])
    views = [p.view for p in outs]
    got = f.apply_obs(fmt, [p.view for p in ins], out=views)
    assert all(g is v for g, v in zip(got, views))
    ctx.sync()
    for i, p in enumerate(ins):
        assert p.unchanged(), "%s: input plane %d changed" % (what, i)
    assert_outputs(outs, e["want"], what)


@pytest.mark.parametrize("fc", CASES + FULL_CASES, ids=case_id)
def test_apply_obs_bit_exact(ctx, fc):
    """Every sharpness of the case through the C-ABI into planes of guard bytes: tight planes, then pitches + 1 / + 13 / + 2 and bases 1 .. 3 bytes off a
    dword, in and (in the reverse order) out."""
    fmt, size = fc
    for s in sharpness_of(size):
        f = new_filter(ctx, s)
        apply_guarded(ctx, f, fmt, size, what="%s s=%g tight" % (case_id(fc), s))
        if size != FULL:
            apply_guarded(ctx, f, fmt, size, pads=(1, 13, 2), offsets=(1, 2, 3), what="%s s=%g padded" % (case_id(fc), s))


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_call_equals_the_three_call_chain_on_the_device(ctx, fmt):
    import torch
    for size in sizes_of(fmt):
        for s in SHARPNESS:
            e = expected(fmt, size, s)
            planes = [gpu(p) for p in e["planes"]]
            f = new_filter(ctx, s)
            one = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
            chained = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
            f.apply_obs(fmt, planes, out=one)
            frame = ctx.ingest_obs(fmt, planes)
            sharp = f.apply(frame) if fmt == "Y800" else f.apply(frame, frame_format(fmt))
            ctx.egress_obs(fmt, sharp, chained)
            ctx.sync()
            for i, (x, y, w) in enumerate(zip(one, chained, e["want"])):
                assert torch.equal(x, y), (fmt, size, s, i)
                assert np.array_equal(x.cpu().numpy(), w), (fmt, size, s, i)


@pytest.mark.parametrize("size", [(9, 14), (9, 13), (17, 35), (67, 257)], ids=lambda s: "%dx%d" % s)
def test_ayuv_planes_based_at_an_odd_byte(ctx, size):
    """No route ends in lvk_hip_egress_obs: the source loads and the sink stores dwords (16 bytes) only where the address allows.  The pad goes to the
    input AND the output plane (apply_guarded reverses the pads for the outputs): with an odd output pitch the rows of one frame alternate between the
    16-byte store, the sink's dword stores and its byte stores inside one launch."""
    f = new_filter(ctx, 0.8)
    for off, pad in ((1, 0), (3, 1), (2, 2), (1, 7), (16, 0), (0, 1), (16, 3)):
        apply_guarded(ctx, f, "AYUV", size, pads=(pad, 0, pad), offsets=(off, 0, off), what="AYUV +%d pad %d" % (off, pad))


@pytest.mark.parametrize("fmt", ["I422", "YUY2", "YVYU", "UYVY", "I444", "BGR3", "Y800", "I420", "NV12"])
@pytest.mark.parametrize("align", [((0, 0, 0), (1, 0, 0)), ((1, 1, 1), (2, 1, 1)), ((13, 13, 1), (3, 1, 2)), ((0, 13, 13), (0, 1, 1)), ((1, 0, 13), (2, 2, 3))],
                         ids=lambda a: "p%d.%d.%d-o%d.%d.%d" % (*a[0], *a[1]))
def test_padded_pitches_and_offsets_keep_their_guard_bytes(ctx, fmt, align):
    """The byte paths of the loads and the stores: every plane at its own pitch and first byte, at a size with a partial last group and at one on the
    far side of the 256-column strip."""
    pads, offsets = align
    f = new_filter(ctx, 0.8)
    for size in (sizes_of(fmt)[2], sizes_of(fmt)[-1]):
        apply_guarded(ctx, f, fmt, size, pads=pads, offsets=offsets, what="%s %s %s" % (fmt, size, align))


def as_i420(planes):
    return planes[0], np.ascontiguousarray(planes[1][..., 0]), np.ascontiguousarray(planes[1][..., 1])


@pytest.mark.parametrize("size", sizes_of("I420"), ids=lambda s: "%dx%d" % s)
def test_i420_and_nv12_give_the_same_samples(ctx, size):
    for s in SHARPNESS:
        f = new_filter(ctx, s)
        a, b = expected("I420", size, s), expected("NV12", size, s)
        assert all(np.array_equal(x, y) for x, y in zip(a["planes"], as_i420(b["planes"])))
        ga = f.apply_yuv420(*[gpu(p) for p in a["planes"]])
        gb = f.apply_yuv420(*[gpu(p) for p in b["planes"]])
        ctx.sync()
        assert len(ga) == 3 and len(gb) == 2
        got_a, got_b = [g.cpu().numpy() for g in ga], as_i420([g.cpu().numpy() for g in gb])
        for i in range(3):
            assert np.array_equal(got_a[i], got_b[i]) and np.array_equal(got_a[i], a["want"][i]), (size, s, i)


@pytest.mark.parametrize("fmt", ["I40A", "I42A", "YUVA"])
def test_the_alpha_plane_is_not_touched(ctx, fmt):
    """The entry takes three planes: a fourth buffer that lies right behind the third output plane -- where OBS keeps the alpha plane -- stays as it is."""
    import torch
    ALPHA = 0xA7
    for size in sizes_of(fmt)[1:]:
        e = expected(fmt, size, 0.8)
        sizes = [w.size for w in e["want"]]
        whole = torch.full((sum(sizes) + size[0] * size[1],), ALPHA, dtype=torch.uint8, device="cuda")
        outs, at = [], 0
        for w in e["want"]:
            outs.append(whole[at:at + w.size].view(w.shape))
            at += w.size
        new_filter(ctx, 0.8).apply_obs(fmt, [gpu(p) for p in e["planes"]], out=outs)
        ctx.sync()
        assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs, e["want"])), size
        assert bool((whole[at:] == ALPHA).all()), size


@pytest.mark.parametrize("fmt", ["I422", "YUY2", "I444", "AYUV", "BGR3", "RGBA", "Y800", "I420", "NV12"])
def test_refused_calls_change_nothing(ctx, fmt):
    size = mid(fmt)
    rows, cols = size
    vf = ctx.VIDEO_FORMATS[fmt]
    e = expected(fmt, size, 0.8)
    pad = 0 if fmt in DIRECT4 else 4
    ins = [Buf(p, pad, 0, seed=20 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], (pad,) * 3)
    n = len(ins)
    ip, isteps = [p.view.data_ptr() for p in ins], [p.pitch for p in ins]
    op, osteps = [p.view.data_ptr() for p in outs], [p.pitch for p in outs]
    irow, orow = [p.row for p in ins], [p.row for p in outs]
    prows = [p.shape[0] for p in ins]
    fn = raw_fn(ctx, "lvk_hip_cas_obs", SIGNATURE)

    def call(handle=ctx.handle, vf=vf, ip=ip, isteps=isteps, op=op, osteps=osteps, rows=rows, cols=cols, sharpness=0.8, null=()):
        a = [None if "ip" in null else arr3(ip, _P), None if "isteps" in null else arr3(isteps, _I),
             None if "op" in null else arr3(op, _P), None if "osteps" in null else arr3(osteps, _I)]
        return fn(handle, vf, a[0], a[1], a[2], a[3], rows, cols, sharpness)

    def unchanged():
        ctx.sync()
        return all(p.unchanged() for p in outs) and all(p.unchanged() for p in ins)

    refused = [dict(handle=None), dict(null=("ip",)), dict(null=("isteps",)), dict(null=("op",)), dict(null=("osteps",))]
    refused += [dict(vf=v) for v in (0, 17, -1, 99)]                                # an unknown format
    refused += [dict(rows=0), dict(cols=0), dict(rows=-2), dict(cols=-2)]
    refused += [dict(sharpness=s) for s in (-0.01, 1.01, float("nan"), float("inf"))]
    if fmt in F422 or fmt in F420:
        refused += [dict(cols=cols - 1), dict(cols=cols + 1)]                       # odd cols
    if fmt in F420:
        refused += [dict(rows=rows - 1), dict(rows=rows + 1)]                       # odd rows
    for i in range(n):
        refused.append(dict(ip=ip[:i] + [None] + ip[i + 1:]))                       # a NULL plane that is in use
        refused.append(dict(op=op[:i] + [None] + op[i + 1:]))
        refused.append(dict(isteps=isteps[:i] + [irow[i] - 1] + isteps[i + 1:]))    # a pitch below its row
        refused.append(dict(osteps=osteps[:i] + [orow[i] - 1] + osteps[i + 1:]))
        refused.append(dict(osteps=osteps[:i] + [1 << 24] + osteps[i + 1:]))        # an output plane 32-bit offsets cannot address
        refused.append(dict(op=op[:i] + [ip[0]] + op[i + 1:]))                      # in place, and ending inside an input plane
        refused.append(dict(op=op[:i] + [ip[n - 1] + isteps[n - 1] * (prows[n - 1] - 1) + irow[n - 1] - 1] + op[i + 1:]))
    if fmt in DIRECT4:
        refused += [dict(isteps=[4 * cols + 4]), dict(osteps=[4 * cols + 4]), dict(isteps=[4 * cols - 4]), dict(osteps=[4 * cols - 4])]
    if n == 3:
        refused.append(dict(op=[op[0], op[0] + osteps[0] * (rows - 1), op[2]]))     # two outputs on each other
        refused.append(dict(op=[op[0], op[1], op[1] + 1]))
    if n == 2:
        refused.append(dict(op=[op[0], op[0] + osteps[0] * (rows - 1)]))
    for a in refused:
        assert call(**a) == ERR_ARG, a
        assert a.get("handle", 1) is None or ctx.lib.lvk_hip_last_error(ctx.handle), a      # every refusal of a live context leaves its message
        assert unchanged(), a

    assert call() == 0
    ctx.sync()
    assert_outputs(outs, e["want"], "after the refusals")
    assert all(p.unchanged() for p in ins)


@pytest.mark.parametrize("nv12", [False, True], ids=["I420", "NV12"])
def test_refused_yuv420_calls_change_nothing(ctx, nv12):
    fmt, size = "NV12" if nv12 else "I420", C_MID_420
    rows, cols = size
    e = expected(fmt, size, 0.8)
    ins = [Buf(p, 4, 0, seed=30 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], (4, 4, 4))
    fn = raw_fn(ctx, "lvk_hip_cas_yuv420", [_P] + [_P, _I] * 6 + [_I, _I, _I, _F])

    def args(bufs):
        a = []
        for p in bufs:
            a += [p.view.data_ptr(), p.pitch]
        return a + [None, 0] * (3 - len(bufs))

    def call(handle=ctx.handle, i=None, o=None, rows=rows, cols=cols, sharpness=0.8):
        return fn(handle, *(i or args(ins)), *(o or args(outs)), rows, cols, 1 if nv12 else 0, sharpness)

    def swapped(a, k, v):
        return a[:k] + [v] + a[k + 1:]

    refused = [dict(handle=None), dict(rows=0), dict(cols=0), dict(rows=rows + 1), dict(cols=cols - 1), dict(sharpness=1.5), dict(sharpness=float("nan"))]
    for k in range(len(ins)):
        refused += [dict(i=swapped(args(ins), 2 * k, None)), dict(o=swapped(args(outs), 2 * k, None)),
                    dict(i=swapped(args(ins), 2 * k + 1, ins[k].row - 1)), dict(o=swapped(args(outs), 2 * k + 1, outs[k].row - 1)),
                    dict(o=swapped(args(outs), 2 * k, ins[0].view.data_ptr()))]
    refused.append(dict(o=swapped(args(outs), 2, outs[0].view.data_ptr() + outs[0].pitch)))      # two outputs on each other
    for a in refused:
        assert call(**a) == ERR_ARG, a
        ctx.sync()
        assert all(p.unchanged() for p in outs) and all(p.unchanged() for p in ins), a
    assert call() == 0
    ctx.sync()
    assert_outputs(outs, e["want"], "after the refusals")
    assert all(p.unchanged() for p in ins)


def test_two_filters_on_one_context(ctx):
    ea, eb = expected("YUY2", (67, 258), 0.0), expected("AYUV", (17, 35), 1.0)
    a, b = new_filter(ctx, 0.0), new_filter(ctx, 1.0)
    pa, pb = [gpu(p) for p in ea["planes"]], [gpu(p) for p in eb["planes"]]
    for _ in range(2):
        ga = a.apply_obs("YUY2", pa)
        gb = b.apply_obs("AYUV", pb)
        ctx.sync()
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(ga, ea["want"]))
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(gb, eb["want"]))
    a.configure(1.0)
    ctx.sync()
    want = expected("YUY2", (67, 258), 1.0)["want"]
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(a.apply_obs("YUY2", pa), want))


def test_the_python_methods_forms(ctx):
    import torch
    import livevisionkit_amd as lvk
    for fmt, size in (("UYVY", (67, 258)), ("I422", (17, 34)), ("Y800", (17, 35)), ("NV12", (18, 34)), ("BGRA", (67, 257)), ("I420", (8, 14))):
        e = expected(fmt, size, 0.8)
        f = new_filter(ctx, 0.8)
        planes = [gpu(p) for p in e["planes"]]
        by_name = f.apply_obs(fmt, planes)
        by_number = f.apply_obs(ctx.VIDEO_FORMATS[fmt], tuple(planes))
        given = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
        back = f.apply_obs(fmt, planes, out=given)
        ctx.sync()
        assert isinstance(by_name, list) and all(b is g for b, g in zip(back, given))
        assert [tuple(a.shape) for a in by_name] == [w.shape for w in e["want"]]
        assert written(fmt, [a.cpu().numpy() for a in by_name], e["want"]) and written(fmt, [a.cpu().numpy() for a in by_number], e["want"])
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(given, e["want"]))
        with pytest.raises(ValueError):
            f.apply_obs(fmt, planes, out=given[:-1] if len(given) > 1 else given + given)
        with pytest.raises(lvk.LvkHipError):
            f.apply_obs(fmt, planes, out=planes)                 # in place
        with pytest.raises(KeyError):
            f.apply_obs("P010", planes)
        if fmt in F420:
            nv12 = fmt == "NV12"
            made = f.apply_yuv420(*planes)                       # v=None: NV12
            given = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
            back = f.apply_yuv420(*planes, out=given) if nv12 else f.apply_yuv420(planes[0], planes[1], v=planes[2], out=given)
            ctx.sync()
            assert isinstance(made, tuple) and len(made) == (2 if nv12 else 3) and all(b is g for b, g in zip(back, given))
            assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(made, e["want"]))
            assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(given, e["want"]))
            with pytest.raises(ValueError):
                f.apply_yuv420(*planes, out=given[:-1])
            with pytest.raises(ValueError):
                f.apply_yuv420(planes[0][:, :-2], *planes[1:])   # planes of two sizes
            with pytest.raises(lvk.LvkHipError):
                f.apply_yuv420(*planes, out=planes)
