"""lvk_hip_fsr_yuv420 / lvk_hip_fsr_obs on the MI355X (csrc/fsr_420.hip, csrc/fsr_obs.hip, csrc/fsr_planes.hpp): the planes of every
OBS video format, out of place, bit for bit against the specification of tests/fsr_obs_cases.py (oracle ingest_obs -> tests/np_fsr.py -> egress_obs; its
liveness: tests/test_fsr_obs_spec.py) and against the GPU's own three-call chain.  Every plane is a view into a buffer of guard bytes (the helpers of
tests/test_lens_obs_gpu.py): pitch padding, what lies before and behind a plane, and the bytes lvk_hip_egress_obs leaves alone (the last quarter of an
RGBA / BGRA / BGRX plane) must come back unchanged, and so must the input planes."""
import ctypes

import numpy as np
import pytest

from tests.fsr_obs_cases import (CASES, CROP_CASES, CROP_FORMATS, DIRECT, DIRECT4, F420, F422, FORMATS, FULL_CASES, GUARD, STAGED, case_id, expected,
                                 first_case, region_of)
from tests.test_lens_obs_gpu import Buf, arr3, assert_outputs, gpu, guarded_outputs, raw_fn, written

pytestmark = pytest.mark.gpu

ERR_ARG = -1
FORMAT_BGR, FORMAT_RGB, FORMAT_YUV = 0, 2, 4
_P, _I = ctypes.c_void_p, ctypes.c_int
SIGNATURE = [_P, _I, _P, _P, _I, _I, _P, _P, _P, _I, _I]
SIGNATURE_420 = [_P] + [_P, _I] * 3 + [_I, _I, _P] + [_P, _I] * 3 + [_I, _I, _I]


def placement(fmt, pads, offsets):
    """The 4-byte DirectIngest planes are tight (steps[0] == 4 * cols); every other plane, AYUV included, takes any pitch and any first byte."""
    return ((0, 0, 0), offsets) if fmt in DIRECT4 else (pads, offsets)


def frame_format(fmt):
    return FORMAT_RGB if fmt == "RGBA" else FORMAT_BGR if fmt in DIRECT4 + ["BGR3"] else FORMAT_YUV


def fsr_obs(ctx, case, ins, outs):
    """lvk_hip_fsr_obs of `case` from the planes `ins` into the planes `outs` (torch tensors)"""
    fmt, src, _, dst = case
    iptr, istep = ctx._obs_args(ins)
    optr, ostep = ctx._obs_args(outs)
    ctx._check(ctx.lib.lvk_hip_fsr_obs(ctx.handle, ctx.VIDEO_FORMATS[fmt], iptr, istep, src[0], src[1], (_I * 4)(*region_of(case)), optr, ostep, dst[0], dst[1]))


def apply_guarded(ctx, case, pads=(0, 0, 0), offsets=(0, 0, 0), what=""):
    e = expected(case)
    pads, offsets = placement(case[0], pads, offsets)
    ins = [Buf(p, pads[i], offsets[i], seed=10 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], pads[::-1], offsets[::-1])
    fsr_obs(ctx, case, [p.view for p in ins], [p.view for p in outs])
    ctx.sync()
    for i, p in enumerate(ins):
        assert p.unchanged(), "%s: input plane %d changed" % (what, i)
    assert_outputs(outs, e["want"], what)


@pytest.mark.parametrize("case", CASES + FULL_CASES, ids=case_id)
def test_fsr_obs_bit_exact(ctx, case):
    """Through the C-ABI into planes of guard bytes: tight planes, then pitches + 1 / + 13 / + 2 and bases 1 .. 3 bytes off a dword, in and (in the
    reverse order) out."""
    apply_guarded(ctx, case, what="%s tight" % case_id(case))
    if case not in FULL_CASES:
        apply_guarded(ctx, case, pads=(1, 13, 2), offsets=(1, 2, 3), what="%s padded" % case_id(case))


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_call_equals_the_three_call_chain_on_the_device(ctx, fmt):
    import torch
    import livevisionkit_amd as lvk
    for path in (STAGED, DIRECT):
        case = first_case(fmt, path)
        _, _, _, dst = case
        e = expected(case)
        planes = [gpu(p) for p in e["planes"]]
        f = lvk.FSRFilter(ctx, output_size=dst, maintain_aspect_ratio=False)
        one = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
        chained = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
        f.apply_obs(fmt, planes, out=one)
        frame = ctx.ingest_obs(fmt, planes)
        scaled = f.apply(frame) if fmt == "Y800" else f.apply(frame, frame_format(fmt))
        ctx.egress_obs(fmt, scaled, chained)
        ctx.sync()
        for i, (x, y, w) in enumerate(zip(one, chained, e["want"])):
            assert torch.equal(x, y), (case_id(case), i)
            assert np.array_equal(x.cpu().numpy(), w), (case_id(case), i)


@pytest.mark.parametrize("fmt", ["I422", "YUY2", "YVYU", "UYVY", "I444", "BGR3", "Y800", "I420", "NV12"])
@pytest.mark.parametrize("align", [((0, 0, 0), (1, 0, 0)), ((1, 1, 1), (2, 1, 1)), ((13, 13, 1), (3, 1, 2)), ((0, 13, 13), (0, 1, 1)), ((1, 0, 13), (2, 2, 3))],
                         ids=lambda a: "p%d.%d.%d-o%d.%d.%d" % (*a[0], *a[1]))
def test_padded_pitches_and_offsets_keep_their_guard_bytes(ctx, fmt, align):
    """The byte paths of the loads and the stores: every plane at its own pitch and first byte, on a staged case with a partial last group and tile and on
    a direct case over several tiles."""
    pads, offsets = align
    for path in (STAGED, DIRECT):
        case = first_case(fmt, path)
        apply_guarded(ctx, case, pads=pads, offsets=offsets, what="%s %s" % (case_id(case), align))


@pytest.mark.parametrize("path", [STAGED, DIRECT], ids=["staged", "direct"])
def test_ayuv_planes_based_at_an_odd_byte(ctx, path):
    """No route ends in lvk_hip_egress_obs: the sink stores dwords (16 bytes) only where the address allows.  The pad goes to the input AND the output
    plane: with an odd output pitch the rows of one frame alternate between the 16-byte store, the sink's dword stores and its byte stores."""
    case = first_case("AYUV", path)
    for off, pad in ((1, 0), (3, 1), (2, 2), (1, 7), (16, 0), (0, 1), (16, 3)):
        apply_guarded(ctx, case, pads=(pad, 0, pad), offsets=(off, 0, off), what="AYUV +%d pad %d" % (off, pad))


def as_i420(planes):
    return planes[0], np.ascontiguousarray(planes[1][..., 0]), np.ascontiguousarray(planes[1][..., 1])


def fsr_yuv420(ctx, case, ins, outs):
    """lvk_hip_fsr_yuv420 of `case` (torch planes; two planes: NV12)"""
    from livevisionkit_amd.context import _planes420_args
    _, src, _, dst = case
    nv12 = len(ins) == 2
    ctx._check(ctx.lib.lvk_hip_fsr_yuv420(ctx.handle, *_planes420_args(tuple(ins), nv12), src[0], src[1], (_I * 4)(*region_of(case)),
                                          *_planes420_args(tuple(outs), nv12), dst[0], dst[1], 1 if nv12 else 0))


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "I420"], ids=case_id)
def test_i420_and_nv12_give_the_same_samples(ctx, case):
    """Through lvk_hip_fsr_yuv420, the entry with the planes as separate arguments."""
    import torch
    nv = ("NV12",) + case[1:]
    a, b = expected(case), expected(nv)
    assert all(np.array_equal(x, y) for x, y in zip(a["planes"], as_i420(b["planes"])))
    ga = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in a["want"]]
    gb = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in b["want"]]
    fsr_yuv420(ctx, case, [gpu(p) for p in a["planes"]], ga)
    fsr_yuv420(ctx, nv, [gpu(p) for p in b["planes"]], gb)
    ctx.sync()
    got_a, got_b = [g.cpu().numpy() for g in ga], as_i420([g.cpu().numpy() for g in gb])
    for i in range(3):
        assert np.array_equal(got_a[i], got_b[i]) and np.array_equal(got_a[i], a["want"][i]), i


@pytest.mark.parametrize("fmt", ["I40A", "I42A", "YUVA"])
def test_the_alpha_plane_is_not_touched(ctx, fmt):
    """The entry takes three planes: a fourth buffer that lies right behind the third output plane -- where OBS keeps the alpha plane -- stays as it is."""
    import torch
    ALPHA = 0xA7
    for path in (STAGED, DIRECT):
        case = first_case(fmt, path)
        e = expected(case)
        sizes = [w.size for w in e["want"]]
        whole = torch.full((sum(sizes) + case[3][0] * case[3][1],), ALPHA, dtype=torch.uint8, device="cuda")
        outs, at = [], 0
        for w in e["want"]:
            outs.append(whole[at:at + w.size].view(w.shape))
            at += w.size
        fsr_obs(ctx, case, [gpu(p) for p in e["planes"]], outs)
        ctx.sync()
        assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs, e["want"])), case_id(case)
        assert bool((whole[at:] == ALPHA).all()), case_id(case)


@pytest.mark.parametrize("fmt", ["I422", "YUY2", "I444", "AYUV", "BGR3", "RGBA", "Y800", "I420", "NV12"])
def test_refused_calls_change_nothing(ctx, fmt):
    case = first_case(fmt, STAGED)
    _, (rows, cols), _, (oh, ow) = case
    vf = ctx.VIDEO_FORMATS[fmt]
    e = expected(case)
    pad = 0 if fmt in DIRECT4 else 4
    ins = [Buf(p, pad, 0, seed=20 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], (pad,) * 3)
    n = len(ins)
    ip, isteps = [p.view.data_ptr() for p in ins], [p.pitch for p in ins]
    op, osteps = [p.view.data_ptr() for p in outs], [p.pitch for p in outs]
    irow, orow = [p.row for p in ins], [p.row for p in outs]
    prows, orows = [p.shape[0] for p in ins], [p.shape[0] for p in outs]
    fn = raw_fn(ctx, "lvk_hip_fsr_obs", SIGNATURE)

    def call(handle=ctx.handle, vf=vf, ip=ip, isteps=isteps, rows=rows, cols=cols, region=(0, 0, cols, rows), op=op, osteps=osteps, oh=oh, ow=ow, null=()):
        a = [None if "ip" in null else arr3(ip, _P), None if "isteps" in null else arr3(isteps, _I),
             None if "op" in null else arr3(op, _P), None if "osteps" in null else arr3(osteps, _I)]
        return fn(handle, vf, a[0], a[1], rows, cols, None if "region" in null else (_I * 4)(*region), a[2], a[3], oh, ow)

    def unchanged():
        ctx.sync()
        return all(p.unchanged() for p in outs) and all(p.unchanged() for p in ins)

    refused = [dict(handle=None), dict(null=("ip",)), dict(null=("isteps",)), dict(null=("op",)), dict(null=("osteps",)), dict(null=("region",))]
    refused += [dict(vf=v) for v in (0, 17, -1, 99)]                                # an unknown format
    refused += [dict(rows=0), dict(cols=0), dict(rows=-2), dict(cols=-2)]
    refused += [dict(oh=0), dict(ow=0), dict(oh=-2), dict(ow=-2)]                   # non-positive output sizes
    # a region that is empty or not inside the frame
    refused += [dict(region=r) for r in ((0, 0, 0, rows), (0, 0, cols, 0), (-1, 0, cols, rows), (0, -1, cols, rows), (1, 0, cols, rows), (0, 1, cols, rows),
                                         (0, 0, cols + 1, rows), (0, 0, cols, rows + 1), (cols, 0, 1, 1), (0, rows, 1, 1), (0, 0, -4, -4),
                                         (2**31 - 1, 0, 2, 2), (0, 2**31 - 1, 2, 2))]
    if fmt in F422 or fmt in F420:
        refused += [dict(cols=cols - 1), dict(cols=cols + 1), dict(ow=ow - 1), dict(ow=ow + 1)]      # odd cols, in and out
    if fmt in F420:
        refused += [dict(rows=rows - 1), dict(rows=rows + 1), dict(oh=oh - 1), dict(oh=oh + 1)]      # odd rows, in and out
    for i in range(n):
        refused.append(dict(ip=ip[:i] + [None] + ip[i + 1:]))                       # a NULL plane that is in use
        refused.append(dict(op=op[:i] + [None] + op[i + 1:]))
        refused.append(dict(isteps=isteps[:i] + [irow[i] - 1] + isteps[i + 1:]))    # a pitch below its row
        refused.append(dict(osteps=osteps[:i] + [orow[i] - 1] + osteps[i + 1:]))
        refused.append(dict(osteps=osteps[:i] + [1 << 24] + osteps[i + 1:]))        # an output plane 32-bit offsets cannot address
        for j in range(n):                                                           # each overlap of an output with an input: at its start, at its end
            refused.append(dict(op=op[:i] + [ip[j]] + op[i + 1:]))
            refused.append(dict(op=op[:i] + [ip[j] + isteps[j] * (prows[j] - 1) + irow[j] - 1] + op[i + 1:]))
            refused.append(dict(op=op[:i] + [ip[j] - (osteps[i] * (orows[i] - 1) + orow[i] - 1)] + op[i + 1:]))
    if fmt in DIRECT4:
        refused += [dict(isteps=[4 * cols + 4]), dict(osteps=[4 * ow + 4]), dict(isteps=[4 * cols - 4]), dict(osteps=[4 * ow - 4])]
    if n == 3:
        refused.append(dict(op=[op[0], op[0] + osteps[0] * (oh - 1), op[2]]))       # two outputs on each other
        refused.append(dict(op=[op[0], op[1], op[1] + 1]))
        refused.append(dict(op=[op[2], op[1], op[2]]))
    if n == 2:
        refused.append(dict(op=[op[0], op[0] + osteps[0] * (oh - 1)]))
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
    case = first_case("NV12" if nv12 else "I420", STAGED)
    _, (rows, cols), _, (oh, ow) = case
    e = expected(case)
    ins = [Buf(p, 4, 0, seed=30 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], (4, 4, 4))
    fn = raw_fn(ctx, "lvk_hip_fsr_yuv420", SIGNATURE_420)

    def args(bufs):
        a = []
        for p in bufs:
            a += [p.view.data_ptr(), p.pitch]
        return a + [None, 0] * (3 - len(bufs))

    def call(handle=ctx.handle, i=None, o=None, rows=rows, cols=cols, region=(0, 0, cols, rows), oh=oh, ow=ow):
        return fn(handle, *(i or args(ins)), rows, cols, None if region is None else (_I * 4)(*region), *(o or args(outs)), oh, ow, 1 if nv12 else 0)

    def swapped(a, k, v):
        return a[:k] + [v] + a[k + 1:]

    refused = [dict(handle=None), dict(region=None), dict(rows=0), dict(cols=0), dict(rows=rows + 1), dict(cols=cols - 1), dict(oh=0), dict(ow=0), dict(oh=-2),
               dict(oh=oh + 1), dict(ow=ow - 1), dict(region=(0, 0, 0, 0)), dict(region=(1, 0, cols, rows)), dict(region=(0, 0, cols, rows + 1)),
               dict(region=(-1, -1, 4, 4))]
    for k in range(len(ins)):
        refused += [dict(i=swapped(args(ins), 2 * k, None)), dict(o=swapped(args(outs), 2 * k, None)),
                    dict(i=swapped(args(ins), 2 * k + 1, ins[k].row - 1)), dict(o=swapped(args(outs), 2 * k + 1, outs[k].row - 1))]
        refused += [dict(o=swapped(args(outs), 2 * k, p.view.data_ptr())) for p in ins]          # each output on each input
    refused.append(dict(o=swapped(args(outs), 2, outs[0].view.data_ptr() + outs[0].pitch)))      # two outputs on each other
    for a in refused:
        assert call(**a) == ERR_ARG, a
        ctx.sync()
        assert all(p.unchanged() for p in outs) and all(p.unchanged() for p in ins), a
    assert call() == 0
    ctx.sync()
    assert_outputs(outs, e["want"], "after the refusals")
    assert all(p.unchanged() for p in ins)


@pytest.mark.parametrize("fmt", ["I420", "UYVY"])
def test_the_direct_route_gives_its_frame_back_to_the_pool(ctx, fmt):
    """The context has no pool diagnostics, so: after one call that lets the pool grow, 50 direct-route calls at 1080p -> 270p (a 6 MB pooled frame each)
    leave torch's allocated bytes where they were and take no more of the device's free memory than one such frame."""
    import torch
    import livevisionkit_amd as lvk
    rows, cols, oh, ow = 1080, 1920, 270, 480
    assert ctx.lib.lvk_hip_fsr_obs_path(cols, rows, oh, ow) == DIRECT
    shapes = {"I420": [(rows, cols), (rows // 2, cols // 2), (rows // 2, cols // 2)], "UYVY": [(rows, cols, 2)]}[fmt]
    oshapes = {"I420": [(oh, ow), (oh // 2, ow // 2), (oh // 2, ow // 2)], "UYVY": [(oh, ow, 2)]}[fmt]
    gen = torch.Generator(device="cuda").manual_seed(5)
    planes = [torch.randint(0, 256, s, dtype=torch.uint8, device="cuda", generator=gen) for s in shapes]
    out = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in oshapes]
    f = lvk.FSRFilter(ctx, output_size=(oh, ow), maintain_aspect_ratio=False)
    f.apply_obs(fmt, planes, out=out)
    ctx.sync()
    first = [o.clone() for o in out]
    allocated, free = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
    for _ in range(50):
        f.apply_obs(fmt, planes, out=out)
    ctx.sync()
    assert torch.cuda.memory_allocated() == allocated
    assert torch.cuda.mem_get_info()[0] >= free - 3 * cols * rows, (free, torch.cuda.mem_get_info()[0])
    assert all(torch.equal(a, b) for a, b in zip(first, out))


def test_two_filters_on_one_context(ctx):
    import livevisionkit_amd as lvk
    ca, cb = first_case("YUY2", STAGED), first_case("AYUV", DIRECT)
    ea, eb = expected(ca), expected(cb)
    a = lvk.FSRFilter(ctx, output_size=ca[3], maintain_aspect_ratio=False)
    b = lvk.FSRFilter(ctx, output_size=cb[3], maintain_aspect_ratio=False)
    pa, pb = [gpu(p) for p in ea["planes"]], [gpu(p) for p in eb["planes"]]
    for _ in range(2):
        ga = a.apply_obs("YUY2", pa)
        gb = b.apply_obs("AYUV", pb)
        ctx.sync()
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(ga, ea["want"]))
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(gb, eb["want"]))
    cc = ("YUY2", (24, 40), None, (18, 30))
    a.configure(output_size=cc[3], maintain_aspect_ratio=False)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(a.apply_obs("YUY2", pa), expected(cc)["want"]))


# (frame rows, cols), region or None, (output rows, cols), the path of the float4 stages (packed, planes), the path of the float stage (gray)
FAMILY_CASES = [((38, 70), (3, 1, 61, 33), (37, 131), STAGED, STAGED),     # partial last tiles in both axes
                ((38, 70), None, (5, 9), STAGED, STAGED),                  # a footprint of nearly the whole frame: 66 x 34 texels still fit
                ((38, 70), None, (16, 64), DIRECT, STAGED),                # one full tile over the whole frame: 72 x 39 float4 texels do not
                ((110, 110), None, (16, 64), DIRECT, DIRECT)]              # ... and 111 x 106 fit neither stage


def test_the_three_kernel_families_agree_on_one_frame(ctx):
    """The packed, the plane and the one-channel kernels walk their tiles with the same code (csrc/fsr_core.hpp): on one frame, lvk_hip_fsr_easu(YUV)
    on the packed pixels equals lvk_hip_fsr_obs(I444) on its three planes byte for byte, and lvk_hip_fsr_easu_gray on plane g equals channel 0 of
    lvk_hip_fsr_easu(BGR) on (g, g, g) (the definition of DESIGN.md section 24), on the staged and on the direct path of each."""
    import torch
    import livevisionkit_amd as lvk
    for (rows, cols), region, dst, path4, path1 in FAMILY_CASES:
        rx, ry, rw, rh = region or (0, 0, cols, rows)
        what = ((rows, cols), region, dst)
        assert ctx.lib.lvk_hip_fsr_easu_path(rw, rh, *dst) == ctx.lib.lvk_hip_fsr_obs_path(rw, rh, *dst) == path4, what
        assert ctx.lib.lvk_hip_fsr_easu_gray_path(rw, rh, *dst) == path1, what
        f = lvk.FSRFilter(ctx, output_size=dst, maintain_aspect_ratio=False, crop=(rx, ry, cols - rx - rw, rows - ry - rh))
        assert tuple(f.geometry(rows, cols)[0]) == (rx, ry, rw, rh), what
        frame = gpu(np.random.default_rng(38).integers(0, 256, (rows, cols, 3), dtype=np.uint8))
        planes = [frame[..., c].contiguous() for c in range(3)]
        packed = f.apply(frame, FORMAT_YUV)
        by_planes = f.apply_obs("I444", planes)
        g = planes[0]
        gray = f.apply(g)
        bgr = f.apply(torch.stack([g, g, g], dim=2), FORMAT_BGR)
        ctx.sync()
        assert tuple(packed.shape) == dst + (3,) and tuple(gray.shape) == dst, what
        for c in range(3):
            assert torch.equal(packed[..., c], by_planes[c]), (what, c)
        assert torch.equal(gray, bgr[..., 0]), what


@pytest.mark.parametrize("fmt", CROP_FORMATS)
def test_the_python_methods_forms(ctx, fmt):
    """The crop settings of the filter reach the entry as the region ((7, 5, 9, 11) of a 24 x 40 frame: crop 7, 5, 24, 8); a skipped frame comes back as it
    is or copied; an output size the format cannot take raises ValueError before anything is enqueued."""
    import torch
    import livevisionkit_amd as lvk
    case = next(c for c in CROP_CASES if c[0] == fmt and c[2] == (7, 5, 9, 11))
    _, (rows, cols), (rx, ry, rw, rh), dst = case
    e = expected(case)
    f = lvk.FSRFilter(ctx, output_size=dst, maintain_aspect_ratio=False, crop=(rx, ry, cols - rx - rw, rows - ry - rh))
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
    # a skip: 1 : 1 on the whole frame
    skip = lvk.FSRFilter(ctx, output_size=(rows, cols), maintain_aspect_ratio=False)
    assert all(a is b for a, b in zip(skip.apply_obs(fmt, planes), planes))
    copies = [torch.full(tuple(p.shape), GUARD, dtype=torch.uint8, device="cuda") for p in planes]
    assert all(a is b for a, b in zip(skip.apply_obs(fmt, planes, out=copies), copies))
    assert all(torch.equal(a, b) for a, b in zip(copies, planes))
    # a refused parity
    if fmt in F420 + F422:
        with pytest.raises(ValueError):
            lvk.FSRFilter(ctx, output_size=(dst[0], dst[1] + 1), maintain_aspect_ratio=False).apply_obs(fmt, planes)
    if fmt in F420:
        nv12 = fmt == "NV12"
        with pytest.raises(ValueError):
            lvk.FSRFilter(ctx, output_size=(dst[0] + 1, dst[1]), maintain_aspect_ratio=False).apply_obs(fmt, planes)
        with pytest.raises(ValueError):
            lvk.FSRFilter(ctx, output_size=(dst[0] + 1, dst[1]), maintain_aspect_ratio=False).apply_yuv420(*planes)
        made = f.apply_yuv420(*planes)                       # v=None: NV12
        given = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
        back = f.apply_yuv420(*planes, out=given) if nv12 else f.apply_yuv420(planes[0], planes[1], v=planes[2], out=given)
        ctx.sync()
        assert isinstance(made, tuple) and len(made) == (2 if nv12 else 3) and all(b is g for b, g in zip(back, given))
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(made, e["want"]))
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(given, e["want"]))
        assert all(a is b for a, b in zip(skip.apply_yuv420(*planes), planes))
        with pytest.raises(ValueError):
            f.apply_yuv420(*planes, out=given[:-1])
        with pytest.raises(ValueError):
            f.apply_yuv420(planes[0][:, :-2], *planes[1:])   # planes of two sizes
