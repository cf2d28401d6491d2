"""lvk_hip_deblock_apply_yuv420 on the MI355X (csrc/deblock_420.hip): I420 and NV12 planes, out of place, bit for bit against
the specification (oracle ingest -> tests/np_deblock.py -> oracle egress; tests/deblock_420_cases.py, whose liveness tests/test_deblock_420_spec.py
asserts) and against the GPU's own three-call chain.  Every plane is a view into a buffer of guard bytes: the pitch padding and what lies before
and behind a plane must come back unchanged, the input planes too."""
import numpy as np
import pytest

from tests import np_deblock as nd
from tests.deblock_420_cases import CASES, as_nv12, case_id, expected, oracle, settings, specification
from tests.deblock_px_cases import blocky

pytestmark = pytest.mark.gpu

ERR_ARG = -1
LAYOUTS = ["i420", "nv12"]
C_SMALL = CASES[6]                      # 66 x 130, region 128 x 64, area tables


def layout_of(planes, layout):
    return as_nv12(planes) if layout == "nv12" else tuple(planes)


class Plane:
    """A plane ([r, c] or, NV12's UV, [r, c, 2]) on the GPU as a view `offset` bytes into a buffer of guard bytes, with a pitch of its row + `pad`."""

    def __init__(self, arr, pad=0, offset=0, fill=None, seed=0):
        import torch
        self.shape = tuple(arr.shape)
        self.row = arr.shape[1] * (2 if arr.ndim == 3 else 1)
        self.pitch, self.offset = self.row + pad, offset
        n = offset + arr.shape[0] * self.pitch + 16
        self.flat = np.full(n, fill, np.uint8) if fill is not None else np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
        if fill is None:
            self.host(self.flat)[...] = arr
        self.buf = torch.from_numpy(self.flat).cuda()
        self.view = self.buf.as_strided(self.shape, (self.pitch, 2, 1) if arr.ndim == 3 else (self.pitch, 1), offset)

    def host(self, flat):
        strides = (self.pitch, 2, 1) if len(self.shape) == 3 else (self.pitch, 1)
        return np.lib.stride_tricks.as_strided(flat[self.offset:], shape=self.shape, strides=strides)

    def expect(self, want):
        out = self.flat.copy()
        self.host(out)[...] = want
        return out

    def equals(self, want):
        return np.array_equal(self.buf.cpu().numpy(), self.expect(want))


def tap_equals(f, info):
    mean, grid, keep = f.grid()
    return np.array_equal(mean, info["mean"]) and np.array_equal(grid, info["grid"]) and np.array_equal(keep, info["keep_block"])


def run(ctx, f, planes, want, pads=(0, 0, 0), in_offsets=(0, 0, 0), out_offsets=(0, 0, 0)):
    """One call on guarded planes; asserts all input and output buffers, returns the region."""
    ins = [Plane(p, pads[i], in_offsets[i], seed=10 + i) for i, p in enumerate(planes)]
    outs = [Plane(p, pads[i], out_offsets[i], fill=0x5A) for i, p in enumerate(planes)]
    res, region = f.apply_yuv420(*[p.view for p in ins], out=[p.view for p in outs])
    ctx.sync()
    for i, (a, b) in enumerate(zip(ins, outs)):
        assert np.array_equal(a.buf.cpu().numpy(), a.flat), "input plane %d changed" % i
        got, exp = b.buf.cpu().numpy(), b.expect(want[i])
        assert np.array_equal(got, exp), "output plane %d: %d bytes differ" % (i, int((got != exp).sum()))
    return region


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_apply_yuv420_bit_exact(ctx, case, layout):
    import livevisionkit_amd as lvk
    e = expected(case)
    f = lvk.DeblockingFilter(ctx, **settings(case))
    region = run(ctx, f, layout_of(e["planes"], layout), layout_of(e["want"], layout))
    assert region == e["info"]["region"] == f.filter_region()
    assert tap_equals(f, e["info"])
    f.close()


def chain(ctx, f, planes, nv12):
    packed = ctx.ingest_yuv420(*planes)
    region = f.apply(packed, nd.FMT_YUV)
    return ctx.egress_yuv420(packed, nv12=nv12), region


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_call_equals_the_three_call_chain(ctx, case, layout):
    import torch
    import livevisionkit_amd as lvk
    e = expected(case)
    planes = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in layout_of(e["planes"], layout)]
    a, b = lvk.DeblockingFilter(ctx, **settings(case)), lvk.DeblockingFilter(ctx, **settings(case))
    got, region = a.apply_yuv420(*planes)
    want, region_chain = chain(ctx, b, planes, layout == "nv12")
    ctx.sync()
    assert region == region_chain
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), i
    for x, y in zip(a.grid(), b.grid()):
        assert np.array_equal(x, y)
    a.close(); b.close()


# Y bases and pitches at every offset from a dword boundary (130 + pad), chroma bases and pitches odd and even: the dword, 16-bit and byte paths of the
# blend's loads and stores, the dword and byte paths of the statistics.  (y pad, chroma pad, y in offset, y out offset, chroma in offset, chroma out offset)
ALIGNMENTS = [(2, 3, 0, 0, 0, 0), (0, 0, 1, 0, 1, 0), (3, 1, 2, 2, 1, 1), (1, 2, 3, 1, 2, 3), (6, 6, 0, 3, 3, 2), (2, 2, 4, 4, 4, 4)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("align", ALIGNMENTS)
def test_padded_pitches_and_offsets_keep_their_guard_bytes(ctx, align, layout):
    import livevisionkit_amd as lvk
    ypad, cpad, yin, yout, cin, cout = align
    e = expected(C_SMALL)
    f = lvk.DeblockingFilter(ctx, **settings(C_SMALL))
    region = run(ctx, f, layout_of(e["planes"], layout), layout_of(e["want"], layout), pads=(ypad, cpad, cpad + 1),
                 in_offsets=(yin, cin, cin + 1), out_offsets=(yout, cout, cout + 3))
    assert region == e["info"]["region"]
    f.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", [CASES[5], CASES[7], CASES[10]], ids=case_id)
def test_every_plane_misaligned(ctx, case, layout):
    # 50 x 38 (region 35 x 50, a last group of two columns, scale 2), 48 x 86 and 130 x 258 (scale 4: the downscale's path of its own, on byte loads here)
    import livevisionkit_amd as lvk
    e = expected(case)
    f = lvk.DeblockingFilter(ctx, **settings(case))
    run(ctx, f, layout_of(e["planes"], layout), layout_of(e["want"], layout), pads=(3, 1, 5), in_offsets=(1, 3, 1), out_offsets=(3, 1, 1))
    f.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_handle_state_is_the_chains(ctx, layout):
    import torch
    import livevisionkit_amd as lvk
    e = expected(C_SMALL)
    rows, cols = C_SMALL[:2]
    planes = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in layout_of(e["planes"], layout)]
    a, b = lvk.DeblockingFilter(ctx, **settings(C_SMALL)), lvk.DeblockingFilter(ctx, **settings(C_SMALL))
    a.apply_yuv420(*planes)
    b.apply(torch.from_numpy(e["packed"].copy()).cuda(), nd.FMT_YUV)
    assert a.filter_region() == b.filter_region() == e["info"]["region"]
    assert tap_equals(a, e["info"]) and tap_equals(b, e["info"])
    img = blocky(rows, cols, seed=77)
    for fmt in (nd.FMT_YUV, nd.FMT_BGR):
        ta, tb = torch.from_numpy(img).cuda(), torch.from_numpy(img).cuda()
        a.draw_influence(ta, fmt); b.draw_influence(tb, fmt)
        ctx.sync()
        assert torch.equal(ta, tb) and np.array_equal(ta.cpu().numpy(), nd.draw_influence(img, fmt, e["info"]))
    a.close(); b.close()


def test_one_handle_alternating_entries_and_sizes(ctx):
    import torch
    import livevisionkit_amd as lvk
    from tests import np_deblock_px as npx
    shared = lvk.DeblockingFilter(ctx)
    o = oracle()
    for rnd, (rows, cols) in enumerate([(66, 130), (48, 86), (66, 130)]):
        # apply (packed), apply_yuv420 (I420), apply_gray, apply_yuv420 (NV12)
        img = blocky(rows, cols, seed=90 + rnd)
        t = torch.from_numpy(img).cuda()
        want, info = nd.deblock(img, nd.FMT_YUV)
        assert shared.apply(t, nd.FMT_YUV) == info["region"]
        ctx.sync()
        assert np.array_equal(t.cpu().numpy(), want) and tap_equals(shared, info)
        for layout in LAYOUTS:
            planes = o.egress_yuv420(blocky(rows, cols, seed=95 + rnd + (layout == "nv12")))
            wantp, infop, _ = specification(planes, 3, 16, 5, 4.0)
            got, region = shared.apply_yuv420(*[torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in layout_of(planes, layout)])
            ctx.sync()
            assert region == infop["region"] and tap_equals(shared, infop)
            for g, w in zip(got, layout_of(wantp, layout)):
                assert np.array_equal(g.cpu().numpy(), w), (rnd, layout)
            if layout == "i420":
                gimg = blocky(rows + 2, cols + 3, seed=99 + rnd, channels=1)
                gt = torch.from_numpy(gimg).cuda()
                gwant, ginfo = npx.deblock_px(gimg, npx.FMT_GRAY)
                assert shared.apply(gt) == ginfo["region"]
                ctx.sync()
                assert np.array_equal(gt.cpu().numpy(), gwant) and tap_equals(shared, ginfo)
    shared.close()


def raw(f, ins, outs, nv12, rows, cols, steps=None):
    """The C entry on raw pointers: ins / outs = three addresses each (None: NULL); steps = the six pitches."""
    return f.lib.lvk_hip_deblock_apply_yuv420(f.handle, ins[0], steps[0], ins[1], steps[1], ins[2], steps[2],
                                              outs[0], steps[3], outs[1], steps[4], outs[2], steps[5], nv12, rows, cols, None)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_refused_calls_change_nothing(ctx, layout):
    import torch
    import livevisionkit_amd as lvk
    case = CASES[7]                                              # 48 x 86, the defaults
    e = expected(case)
    rows, cols = case[:2]
    nv12 = 1 if layout == "nv12" else 0
    planes, want = layout_of(e["planes"], layout), layout_of(e["want"], layout)
    ins = [Plane(p, 4, 0, seed=20 + i) for i, p in enumerate(planes)]
    outs = [Plane(p, 4, 0, fill=0x5A) for p in planes]

    def ptrs(ps):
        return [p.view.data_ptr() for p in ps] + [None] * (3 - len(ps))

    def pitches(ps):
        return [p.pitch for p in ps] + [0] * (3 - len(ps))

    ip, op, steps = ptrs(ins), ptrs(outs), pitches(ins) + pitches(outs)

    fresh = lvk.DeblockingFilter(ctx)
    assert raw(fresh, [None] + ip[1:], op, nv12, rows, cols, steps) == ERR_ARG
    assert fresh.filter_region() == (0, 0, 0, 0)
    with pytest.raises(lvk.LvkHipError):
        fresh.grid()                                             # still nothing applied
    fresh.close()

    f = lvk.DeblockingFilter(ctx)
    f.apply_yuv420(*[p.view for p in ins], out=[p.view for p in outs])
    ctx.sync()
    assert all(p.equals(w) for p, w in zip(outs, want))
    applied = [p.buf.cpu().numpy() for p in outs]

    def unchanged():
        ctx.sync()
        return (all(np.array_equal(p.buf.cpu().numpy(), a) for p, a in zip(outs, applied)) and all(np.array_equal(p.buf.cpu().numpy(), p.flat) for p in ins)
                and f.filter_region() == e["info"]["region"] and tap_equals(f, e["info"]))

    n = len(planes)
    refused = []
    for i in range(n):                                           # a NULL plane that is in use
        refused.append((ip[:i] + [None] + ip[i + 1:], op, rows, cols, steps))
        refused.append((ip, op[:i] + [None] + op[i + 1:], rows, cols, steps))
    for r, c in [(rows + 1, cols), (rows, cols - 1), (0, cols), (rows, 0), (-2, cols), (rows, -2)]:        # odd or non-positive sizes
        refused.append((ip, op, r, c, steps))
    rowbytes = [cols, cols if nv12 else cols // 2, cols // 2]
    for i in range(n):                                           # a pitch smaller than its row
        for base in (0, 3):
            s = list(steps); s[base + i] = rowbytes[i] - 1
            refused.append((ip, op, rows, cols, s))
    # overlaps: an output on its input, an output Y that starts inside the last input plane, an output chroma inside the input Y, two outputs on each other
    refused.append((ip, [ip[0]] + op[1:], rows, cols, steps))
    refused.append((ip, [ip[n - 1] + 7] + op[1:], rows, cols, steps))
    refused.append((ip, [op[0], ip[0] + 5] + op[2:], rows, cols, steps))
    refused.append((ip, [op[0], op[0] + steps[3] * (rows - 1)] + op[2:], rows, cols, steps))
    if not nv12:
        refused.append((ip, [op[0], op[1], op[1] + 1], rows, cols, steps))
        refused.append((ip, [op[0], op[1], ip[1]], rows, cols, steps))
    for a in refused:
        assert raw(f, a[0], a[1], nv12, a[2], a[3], a[4]) == ERR_ARG, a
        assert unchanged(), a
    # NV12 ignores d_v / o_v: whatever they are, the call runs
    if nv12:
        assert raw(f, ip[:2] + [ip[0]], op[:2] + [ip[0]], 1, rows, cols, steps) == 0
        assert unchanged()

    def refused_by_settings(planes_np):
        ps = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes_np]
        os_ = [torch.full_like(p, 0x5A) for p in ps]
        with pytest.raises(lvk.LvkHipError) as err:
            f.apply_yuv420(*ps, out=os_)
        ctx.sync()
        assert all(bool((o == 0x5A).all()) for o in os_)
        return str(err.value)

    o = oracle()
    low = layout_of(o.egress_yuv420(blocky(14, 200, seed=6)), layout)                       # no whole 16 x 16 block
    assert "the frame holds no whole macroblock" in refused_by_settings(low)
    assert unchanged()
    f.configure(filter_size=257)                                 # accepted by configure, refused by apply
    assert "s.filter_size <= (uint32_t)kMaxFilterSize" in refused_by_settings(planes)
    assert unchanged()
    f.configure(block_size=2, filter_scaling=8.0)
    tiny = layout_of(o.egress_yuv420(blocky(2, 2, seed=7)), layout)
    assert "downscale of the region is empty" in refused_by_settings(tiny)                  # rint(2 / 8) = 0
    f.configure()
    assert unchanged()
    f.close()


def test_refusal_messages_are_those_of_apply(ctx):
    import torch
    import livevisionkit_amd as lvk
    f = lvk.DeblockingFilter(ctx)
    msgs = []
    for conf, (rows, cols) in [(dict(), (14, 200)), (dict(filter_size=257), (48, 86)), (dict(block_size=2, filter_scaling=8.0), (2, 2))]:
        f.configure(**conf)
        with pytest.raises(lvk.LvkHipError) as err:
            f.apply(torch.from_numpy(blocky(rows, cols, seed=1)).cuda(), nd.FMT_YUV)
        packed = str(err.value).replace("lvk_hip_deblock_apply", "ENTRY")
        y = torch.zeros((rows, cols), dtype=torch.uint8, device="cuda")
        u = torch.zeros((rows // 2, cols // 2), dtype=torch.uint8, device="cuda")
        with pytest.raises(lvk.LvkHipError) as err:
            f.apply_yuv420(y, u, u.clone())
        msgs.append((packed, str(err.value).replace("lvk_hip_deblock_apply_yuv420", "ENTRY")))
    assert all(a == b for a, b in msgs), msgs
    f.close()


def test_two_filters_on_one_context(ctx):
    import torch
    import livevisionkit_amd as lvk
    ca, cb = CASES[6], CASES[8]
    ea, eb = expected(ca), expected(cb)
    a, b = lvk.DeblockingFilter(ctx, **settings(ca)), lvk.DeblockingFilter(ctx, **settings(cb))
    pa = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in ea["planes"]]
    pb = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in as_nv12(eb["planes"])]
    for _ in range(2):
        ga, ra = a.apply_yuv420(*pa)
        gb, rb = b.apply_yuv420(*pb)
        ctx.sync()
        assert ra == ea["info"]["region"] and rb == eb["info"]["region"]
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(ga, ea["want"]))
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(gb, as_nv12(eb["want"])))
        assert tap_equals(a, ea["info"]) and tap_equals(b, eb["info"])
    a.close(); b.close()
