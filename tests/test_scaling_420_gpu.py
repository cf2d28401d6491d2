"""lvk_hip_scale_yuv420 on the MI355X (csrc/scaling_420.hip): I420 and NV12 planes, out of place, bit for bit against the
specification (oracle ingest -> upscale -> sharpen -> egress; tests/scaling_420_cases.py, whose liveness tests/test_scaling_420_spec.py asserts) and
against the GPU's own four-call chain.  Every plane is a view into a buffer of guard bytes (the Plane of tests/test_deblock_420_gpu.py): the pitch
padding and what lies before and behind a plane must come back unchanged, the input planes too."""
import numpy as np
import pytest

from tests.scaling_420_cases import (C_14x34, C_128, C_258, C_P254, CASES, TEXTURES, case_id, expected, layout_of)
from tests.test_deblock_420_gpu import Plane

pytestmark = pytest.mark.gpu

ERR_ARG = -1
LAYOUTS = ["i420", "nv12"]


def run(ctx, case, planes, want, in_pads=(0, 0, 0), out_pads=(0, 0, 0), in_offsets=(0, 0, 0), out_offsets=(0, 0, 0)):
    """One call on guarded planes; asserts all input and output buffers."""
    ins = [Plane(p, in_pads[i], in_offsets[i], seed=10 + i) for i, p in enumerate(planes)]
    outs = [Plane(w, out_pads[i], out_offsets[i], fill=0x5A) for i, w in enumerate(want)]
    v = ins[2].view if len(ins) == 3 else None
    ctx.scale_yuv420(ins[0].view, ins[1].view, v, size=(case[3], case[2]), sharpness=case[4], out=[p.view for p in outs])
    ctx.sync()
    for i, (a, b) in enumerate(zip(ins, outs)):
        assert np.array_equal(a.buf.cpu().numpy(), a.flat), "input plane %d changed" % i
        got, exp = b.buf.cpu().numpy(), b.expect(want[i])
        assert np.array_equal(got, exp), "output plane %d: %d bytes differ" % (i, int((got != exp).sum()))


def gpu_planes(planes):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes]


def four_calls(ctx, planes, case, nv12):
    packed = ctx.ingest_yuv420(*planes)
    scaled = ctx.upscale(packed, (case[3], case[2]), yuv=True)
    return ctx.egress_yuv420(ctx.sharpen(scaled, case[4]), nv12=nv12)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_scale_yuv420_bit_exact_and_equal_to_the_four_call_chain(ctx, case, layout):
    import torch
    for kind in TEXTURES:
        e = expected(case, kind)
        planes, want = layout_of(e["planes"], layout), layout_of(e["want"], layout)
        run(ctx, case, planes, want)
        dev = gpu_planes(planes)
        got = ctx.scale_yuv420(*dev, size=(case[3], case[2]), sharpness=case[4])
        chained = four_calls(ctx, dev, case, layout == "nv12")
        ctx.sync()
        assert len(got) == len(chained) == len(want)
        for i, (g, c) in enumerate(zip(got, chained)):
            assert torch.equal(g, c), (kind, i)


# Y bases and pitches at every offset from a dword boundary, chroma bases and pitches odd and even, pitch pads 0 / 1 / 13 on inputs and outputs: the
# dword, 16-bit and byte paths of the loads and stores.  (Y in pad, chroma in pad, Y out pad, chroma out pad, Y in offset, Y out offset, chroma in
# offset, chroma out offset)
ALIGNMENTS = [(0, 0, 0, 0, 1, 0, 1, 0), (1, 13, 0, 1, 0, 1, 0, 1), (13, 1, 1, 0, 2, 2, 2, 2), (0, 1, 13, 13, 3, 3, 1, 3), (2, 2, 2, 2, 0, 0, 0, 0),
              (13, 0, 1, 13, 3, 1, 3, 2), (1, 1, 0, 0, 0, 2, 4, 1)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("align", ALIGNMENTS)
@pytest.mark.parametrize("case", [C_14x34, C_258, C_P254], ids=case_id)
def test_padded_pitches_and_offsets_keep_their_guard_bytes(ctx, case, align, layout):
    yip, cip, yop, cop, yin, yout, cin, cout = align
    e = expected(case, "random")
    run(ctx, case, layout_of(e["planes"], layout), layout_of(e["want"], layout), in_pads=(yip, cip, cip + 1), out_pads=(yop, cop, cop + 3),
        in_offsets=(yin, cin, cin + 1), out_offsets=(yout, cout, cout + 3))


def test_one_context_alternates_routes_and_sizes(ctx):
    # the scratch frames of the upscale route go back to the context's pool inside every call and are handed out again, at changing sizes
    for rnd in range(12):
        case = [C_128, C_P254, C_14x34][rnd % 3]
        layout = LAYOUTS[(rnd // 3) % 2]
        e = expected(case, TEXTURES[rnd % 2])
        got = ctx.scale_yuv420(*gpu_planes(layout_of(e["planes"], layout)), size=(case[3], case[2]), sharpness=case[4])
        ctx.sync()
        for i, (g, w) in enumerate(zip(got, layout_of(e["want"], layout))):
            assert np.array_equal(g.cpu().numpy(), w), (rnd, i)


def test_two_contexts_run_the_same_case(ctx):
    import livevisionkit_amd as lvk
    other = lvk.Context(0)
    e = expected(C_258, "smooth")
    dev = gpu_planes(e["planes"])
    ctx.sync()
    for _ in range(2):
        a = ctx.scale_yuv420(*dev, size=(C_258[3], C_258[2]), sharpness=C_258[4])
        b = other.scale_yuv420(*dev, size=(C_258[3], C_258[2]), sharpness=C_258[4])
        ctx.sync(); other.sync()
        for x, y, w in zip(a, b, e["want"]):
            assert np.array_equal(x.cpu().numpy(), w) and np.array_equal(y.cpu().numpy(), w)
    other.close()


def raw(ctx, ins, in_steps, src, outs, out_steps, dst, nv12, sharpness):
    """The C entry on raw pointers: ins / outs = three addresses each (None: NULL), three pitches each, src / dst = (rows, cols)."""
    return ctx.lib.lvk_hip_scale_yuv420(ctx.handle, ins[0], in_steps[0], ins[1], in_steps[1], ins[2], in_steps[2], src[0], src[1],
                                        outs[0], out_steps[0], outs[1], out_steps[1], outs[2], out_steps[2], dst[0], dst[1], nv12, sharpness)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", [C_14x34, CASES[17]], ids=case_id)
def test_refused_calls_change_nothing(ctx, case, layout):
    e = expected(case, "random")
    src, dst, sharpness = case[:2], case[2:4], case[4]
    nv12 = 1 if layout == "nv12" else 0
    planes, want = layout_of(e["planes"], layout), layout_of(e["want"], layout)
    ins = [Plane(p, 4, 0, seed=20 + i) for i, p in enumerate(planes)]
    outs = [Plane(w, 4, 0, fill=0x5A) for w in want]
    n = len(planes)

    def ptrs(ps):
        return [p.view.data_ptr() for p in ps] + [None] * (3 - len(ps))

    def pitches(ps):
        return [p.pitch for p in ps] + [0] * (3 - len(ps))

    ip, op, isteps, osteps = ptrs(ins), ptrs(outs), pitches(ins), pitches(outs)
    before = [p.buf.cpu().numpy() for p in outs]

    def unchanged():
        ctx.sync()
        return (all(np.array_equal(p.buf.cpu().numpy(), b) for p, b in zip(outs, before)) and all(np.array_equal(p.buf.cpu().numpy(), p.flat) for p in ins))

    refused = []                                                 # (ins, in steps, src, outs, out steps, dst, sharpness)
    for i in range(n):                                           # a NULL plane that is in use
        refused.append((ip[:i] + [None] + ip[i + 1:], isteps, src, op, osteps, dst, sharpness))
        refused.append((ip, isteps, src, op[:i] + [None] + op[i + 1:], osteps, dst, sharpness))
    for bad in [1, 0, -2, 3]:                                    # any of the four sizes odd or below 2
        refused.append((ip, isteps, (bad, src[1]), op, osteps, dst, sharpness))
        refused.append((ip, isteps, (src[0], bad), op, osteps, dst, sharpness))
        refused.append((ip, isteps, src, op, osteps, (bad, dst[1]), sharpness))
        refused.append((ip, isteps, src, op, osteps, (dst[0], bad), sharpness))
    refused.append((ip, isteps, (src[0] + 1, src[1]), op, osteps, (dst[0] + 1, dst[1]), sharpness))
    refused.append((ip, isteps, src, op, osteps, (src[0] - 2, dst[1]), sharpness))         # a destination smaller than the source
    refused.append((ip, isteps, src, op, osteps, (dst[0], src[1] - 2), sharpness))
    in_row = [src[1], src[1] if nv12 else src[1] // 2, src[1] // 2]
    out_row = [dst[1], dst[1] if nv12 else dst[1] // 2, dst[1] // 2]
    for i in range(n):                                           # a pitch smaller than its row
        s = list(isteps); s[i] = in_row[i] - 1
        refused.append((ip, s, src, op, osteps, dst, sharpness))
        s = list(osteps); s[i] = out_row[i] - 1
        refused.append((ip, isteps, src, op, s, dst, sharpness))
    for bad in [-0.01, 1.01, float("nan"), float("inf"), -float("inf")]:                    # a sharpness outside [0, 1]
        refused.append((ip, isteps, src, op, osteps, dst, bad))
    # overlaps: an output on its input, an output Y that starts inside the last input plane, an output chroma inside the input Y, two outputs on each other
    refused.append((ip, isteps, src, [ip[0]] + op[1:], osteps, dst, sharpness))
    refused.append((ip, isteps, src, [ip[n - 1] + 7] + op[1:], osteps, dst, sharpness))
    refused.append((ip, isteps, src, [op[0], ip[0] + 5] + op[2:], osteps, dst, sharpness))
    refused.append((ip, isteps, src, [op[0], op[0] + osteps[0] * (dst[0] - 1)] + op[2:], osteps, dst, sharpness))
    if not nv12:
        refused.append((ip, isteps, src, [op[0], op[1], op[1] + 1], osteps, dst, sharpness))
        refused.append((ip, isteps, src, [op[0], op[1], ip[1]], osteps, dst, sharpness))
    for a in refused:
        assert raw(ctx, a[0], a[1], a[2], a[3], a[4], a[5], nv12, a[6]) == ERR_ARG, a
        assert unchanged(), a
    assert ctx.lib.lvk_hip_scale_yuv420(None, ip[0], isteps[0], ip[1], isteps[1], ip[2], isteps[2], src[0], src[1],
                                        op[0], osteps[0], op[1], osteps[1], op[2], osteps[2], dst[0], dst[1], nv12, sharpness) == ERR_ARG
    assert unchanged()
    # the next valid call is correct; NV12 ignores d_v / o_v, whatever they are
    assert raw(ctx, ip[:2] + [ip[0]] if nv12 else ip, isteps, src, op[:2] + [ip[0]] if nv12 else op, osteps, dst, nv12, sharpness) == 0
    ctx.sync()
    assert all(p.equals(w) for p, w in zip(outs, want))
    assert all(np.array_equal(p.buf.cpu().numpy(), p.flat) for p in ins)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_python_method_forms(ctx, layout):
    import torch
    import livevisionkit_amd as lvk
    # returned planes: the layout follows the input's; size=None sharpens at the input's size
    for case in (C_14x34, C_P254):
        e = expected(case, "smooth")
        dev = gpu_planes(layout_of(e["planes"], layout))
        got = ctx.scale_yuv420(*dev, size=None if case is C_P254 else (case[3], case[2]))
        ctx.sync()
        want = layout_of(e["want"], layout)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == torch.uint8 and tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w)
        # out=: the same tensors come back, written
        outs = [torch.full(w.shape, 0x5A, dtype=torch.uint8, device="cuda") for w in want]
        back = ctx.scale_yuv420(*dev, size=(case[3], case[2]), sharpness=0.8, out=outs)
        ctx.sync()
        assert all(b is o for b, o in zip(back, outs))
        assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs, want))
    # a refusal raises
    e = expected(C_14x34, "smooth")
    dev = gpu_planes(layout_of(e["planes"], layout))
    with pytest.raises(lvk.LvkHipError):
        ctx.scale_yuv420(*dev, size=(C_14x34[1] - 2, C_14x34[0]))
    with pytest.raises(lvk.LvkHipError):
        ctx.scale_yuv420(*dev, size=(C_14x34[3], C_14x34[2]), sharpness=1.5)
