"""lvk_hip_deblock_apply_obs on the MI355X (csrc/deblock_obs.hip): the planes of every OBS video format, out of place, bit for bit
against the specification of tests/deblock_obs_cases.py (oracle ingest_obs -> tests/np_deblock.py -> egress_obs; its liveness:
tests/test_deblock_obs_spec.py) and against the GPU's own three-call chain.  Every plane is a view into a buffer of guard bytes (the helpers of
tests/test_lens_obs_gpu.py): pitch padding, what lies before and behind a plane, and the bytes lvk_hip_egress_obs leaves alone (the last quarter of an
RGBA / BGRA / BGRX plane) must come back unchanged, and so must the input planes."""
import ctypes

import numpy as np
import pytest

from tests import np_deblock as nd
from tests.deblock_obs_cases import (ALL_CASES, CASES_420, CASES_EVEN, CASES_ODD, DIRECT4, F420, F422, FORMATS, FRAME_YUV, GUARD, case_id, cases_of, expected,
                                     frame_format, inputs, settings)
from tests.deblock_px_cases import blocky
from tests.test_deblock_420_gpu import tap_equals
from tests.test_lens_obs_gpu import Buf, arr3, assert_outputs, gpu, guarded_outputs, raw_fn, written

pytestmark = pytest.mark.gpu

ERR_ARG = -1
_P, _I = ctypes.c_void_p, ctypes.c_int
SIGNATURE = [_P, _I, _P, _P, _P, _P, _I, _I, _P]
C_DEFAULTS = (48, 86, 3, 16, 5, 4.0)                   # a case of every format, at the default settings
C_TABLES = (66, 130, 3, 16, 5, 3.0)


def placement(fmt, pads, offsets):
    """The 4-byte DirectIngest planes are tight (steps[0] == 4 * cols); every other plane, AYUV included, takes any pitch and any first byte."""
    return ((0, 0, 0), offsets) if fmt in DIRECT4 else (pads, offsets)


def new_filter(ctx, case):
    import livevisionkit_amd as lvk
    return lvk.DeblockingFilter(ctx, **settings(case))


def apply_guarded(ctx, f, fmt, case, pads=(0, 0, 0), offsets=(0, 0, 0), what=""):
    e = expected(fmt, case)
    pads, offsets = placement(fmt, pads, offsets)
    ins = [Buf(p, pads[i], offsets[i], seed=10 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], pads, offsets[::-1])
    views = [p.view for p in outs]
    got, region = f.apply_obs(fmt, [p.view for p in ins], out=views)
    assert all(g is v for g, v in zip(got, views))
    ctx.sync()
    for i, p in enumerate(ins):
        assert p.unchanged(), "%s: input plane %d changed" % (what, i)
    assert_outputs(outs, e["want"], what)
    assert region == e["info"]["region"] == f.filter_region()
    return region


@pytest.mark.parametrize("fc", ALL_CASES, ids=case_id)
def test_apply_obs_bit_exact(ctx, fc):
    """Through the C-ABI into planes of guard bytes: tight planes, then pitches + 1 / + 13 / + 2 and bases 1 .. 3 bytes off a dword; the taps too."""
    fmt, case = fc
    f = new_filter(ctx, case)
    apply_guarded(ctx, f, fmt, case, what=case_id(fc) + " tight")
    if case[0] < 1080:
        apply_guarded(ctx, f, fmt, case, pads=(1, 13, 2), offsets=(1, 2, 3), what=case_id(fc) + " padded")
    assert tap_equals(f, expected(fmt, case)["info"])
    f.close()


def three_of(fmt):
    c = cases_of(fmt)
    return [c[3], c[6], c[7]] if fmt in F420 else [c[3], c[5], c[9]]


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_call_equals_the_three_call_chain_on_the_device(ctx, fmt):
    import torch
    for case in three_of(fmt):
        e = expected(fmt, case)
        planes = [gpu(p) for p in e["planes"]]
        a, b = new_filter(ctx, case), new_filter(ctx, case)
        one = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
        chained = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
        _, region = a.apply_obs(fmt, planes, out=one)
        frame = ctx.ingest_obs(fmt, planes)
        region_chain = b.apply(frame) if fmt == "Y800" else b.apply(frame, frame_format(fmt))
        ctx.egress_obs(fmt, frame, chained)
        ctx.sync()
        assert region == region_chain == e["info"]["region"]
        for i, (x, y, w) in enumerate(zip(one, chained, e["want"])):
            assert torch.equal(x, y), (fmt, case, i)
            assert np.array_equal(x.cpu().numpy(), w), (fmt, case, i)
        for x, y in zip(a.grid(), b.grid()):
            assert np.array_equal(x, y)
        a.close(); b.close()


@pytest.mark.parametrize("case", [CASES_EVEN[2], CASES_EVEN[5], CASES_ODD[2], CASES_ODD[3]], ids=lambda c: "%dx%d" % c[:2])
def test_ayuv_planes_based_at_an_odd_byte(ctx, case):
    """No route ends in lvk_hip_egress_obs: the source loads and the sink stores dwords (16 bytes) only where the address allows."""
    f = new_filter(ctx, case)
    for off, pad in ((1, 0), (3, 1), (2, 2), (1, 7), (16, 0)):
        apply_guarded(ctx, f, "AYUV", case, pads=(pad, 0, 0), offsets=(off, 0, off), what="AYUV +%d pad %d" % (off, pad))
    f.close()


@pytest.mark.parametrize("fmt", ["UYVY", "I444"])
def test_handle_state_is_the_chains(ctx, fmt):
    import torch
    case = C_TABLES
    e = expected(fmt, case)
    rows, cols = case[:2]
    a, b = new_filter(ctx, case), new_filter(ctx, case)
    a.apply_obs(fmt, [gpu(p) for p in e["planes"]])
    b.apply(torch.from_numpy(e["packed"].copy()).cuda(), nd.FMT_YUV)
    assert a.filter_region() == b.filter_region() == e["info"]["region"]
    assert tap_equals(a, e["info"]) and tap_equals(b, e["info"])
    img = blocky(rows, cols, seed=77)
    for pf in (nd.FMT_YUV, nd.FMT_BGR):
        ta, tb = torch.from_numpy(img).cuda(), torch.from_numpy(img).cuda()
        a.draw_influence(ta, pf); b.draw_influence(tb, pf)
        ctx.sync()
        assert torch.equal(ta, tb) and np.array_equal(ta.cpu().numpy(), nd.draw_influence(img, pf, e["info"]))
    a.close(); b.close()


def test_one_handle_alternating_entries_sizes_and_formats(ctx):
    """apply_obs on three formats, apply_yuv420 and the packed apply, at two sizes, on one handle at the default settings"""
    import torch
    import livevisionkit_amd as lvk
    from tests import deblock_420_cases as c420
    shared = lvk.DeblockingFilter(ctx)
    big, small = (66, 254, 3, 16, 5, 4.0), C_DEFAULTS
    steps = 0
    for rnd in range(2):
        for fmt, case in [("UYVY", big), ("packed", small), ("I444", small), ("420", small), ("BGRA", big), ("UYVY", small), ("packed", big), ("NV12", small),
                          ("Y800", big), ("AYUV", small)]:
            rows, cols = case[:2]
            if fmt == "packed":
                img = blocky(rows, cols, seed=90 + rnd)
                t = torch.from_numpy(img).cuda()
                want, info = nd.deblock(img, nd.FMT_YUV)
                assert shared.apply(t, nd.FMT_YUV) == info["region"]
                ctx.sync()
                assert np.array_equal(t.cpu().numpy(), want) and tap_equals(shared, info)
            elif fmt == "420":
                e = c420.expected(case)
                got, region = shared.apply_yuv420(*[gpu(p) for p in e["planes"]])
                ctx.sync()
                assert region == e["info"]["region"] and tap_equals(shared, e["info"])
                assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, e["want"]))
            else:
                e = expected(fmt, case)
                got, region = shared.apply_obs(fmt, [gpu(p) for p in e["planes"]])
                ctx.sync()
                assert region == e["info"]["region"] and tap_equals(shared, e["info"]), (fmt, case)
                assert written(fmt, [g.cpu().numpy() for g in got], e["want"]), (fmt, case)
            steps += 1
    assert steps == 20
    shared.close()


@pytest.mark.parametrize("fmt", ["I422", "YUY2", "I444", "AYUV", "BGR3", "RGBA", "Y800", "I420", "NV12"])
def test_refused_calls_change_nothing(ctx, fmt):
    import livevisionkit_amd as lvk
    case = C_DEFAULTS
    rows, cols = case[:2]
    vf = ctx.VIDEO_FORMATS[fmt]
    e = expected(fmt, case)
    pad = 0 if fmt in DIRECT4 else 4
    ins = [Buf(p, pad, 0, seed=20 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], (pad,) * 3)
    n = len(ins)
    ip, isteps = [p.view.data_ptr() for p in ins], [p.pitch for p in ins]
    op, osteps = [p.view.data_ptr() for p in outs], [p.pitch for p in outs]
    irow, orow = [p.row for p in ins], [p.row for p in outs]
    prows = [p.shape[0] for p in ins]
    fn = raw_fn(ctx, "lvk_hip_deblock_apply_obs", SIGNATURE)

    fresh = lvk.DeblockingFilter(ctx)
    assert fn(fresh.handle, vf, arr3([None] + ip[1:], _P), arr3(isteps, _I), arr3(op, _P), arr3(osteps, _I), rows, cols, None) == ERR_ARG
    assert fresh.filter_region() == (0, 0, 0, 0)
    with pytest.raises(lvk.LvkHipError):
        fresh.grid()                                             # still nothing applied
    fresh.close()

    # the handle's state comes from a frame of another size: a refused call must leave region, maps and taps at that
    f = lvk.DeblockingFilter(ctx)
    before = expected("I444", C_TABLES)
    f.apply_obs("I444", [gpu(p) for p in before["planes"]])
    region = (ctypes.c_int * 4)(-7, -7, -7, -7)

    def call(vf=vf, ip=ip, isteps=isteps, op=op, osteps=osteps, rows=rows, cols=cols, null=()):
        a = [None if "ip" in null else arr3(ip, _P), None if "isteps" in null else arr3(isteps, _I),
             None if "op" in null else arr3(op, _P), None if "osteps" in null else arr3(osteps, _I)]
        return fn(None if "handle" in null else f.handle, vf, a[0], a[1], a[2], a[3], rows, cols, region)

    def unchanged():
        ctx.sync()
        return (all(p.unchanged() for p in outs) and all(p.unchanged() for p in ins) and tuple(region) == (-7, -7, -7, -7)
                and f.filter_region() == before["info"]["region"] and tap_equals(f, before["info"]))

    refused = [dict(null=("handle",)), dict(null=("ip",)), dict(null=("isteps",)), dict(null=("op",)), dict(null=("osteps",))]
    refused += [dict(vf=v) for v in (0, 17, -1, 99)]                                # an unknown format
    refused += [dict(rows=0), dict(cols=0), dict(rows=-2), dict(cols=-2)]
    if fmt in F422 or fmt in F420:
        refused += [dict(cols=cols - 1), dict(cols=cols + 1)]                       # odd cols
    if fmt in F420:
        refused += [dict(rows=rows - 1), dict(rows=rows + 1)]                       # odd rows
    for i in range(n):
        refused.append(dict(ip=ip[:i] + [None] + ip[i + 1:]))                       # a NULL plane that is in use
        refused.append(dict(op=op[:i] + [None] + op[i + 1:]))
        refused.append(dict(isteps=isteps[:i] + [irow[i] - 1] + isteps[i + 1:]))    # a pitch below its row
        refused.append(dict(osteps=osteps[:i] + [orow[i] - 1] + osteps[i + 1:]))
        if fmt not in F420:                                                         # an output plane the sinks' 32-bit offsets cannot address
            refused.append(dict(osteps=osteps[:i] + [1 << 24] + osteps[i + 1:]))
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
        assert "handle" in a.get("null", ()) or ctx.lib.lvk_hip_last_error(ctx.handle), a      # every refusal of a live handle leaves its message
        assert unchanged(), a

    # apply's three refusals, in apply's own words
    def refused_by_settings(shape_case, conf):
        f.configure(**conf)
        tight = dict(isteps=[4 * shape_case[1]], osteps=[4 * shape_case[1]]) if fmt in DIRECT4 else {}       # DirectIngest's pitch is 4 * cols
        rc = call(rows=shape_case[0], cols=shape_case[1], **tight)
        msg = ctx.lib.lvk_hip_last_error(ctx.handle)
        f.configure()
        assert rc == ERR_ARG and unchanged(), conf
        return msg.decode() if isinstance(msg, bytes) else str(msg)

    assert "the frame holds no whole macroblock" in refused_by_settings((rows, cols), dict(block_size=64))
    assert "s.filter_size <= (uint32_t)kMaxFilterSize" in refused_by_settings((rows, cols), dict(filter_size=257))
    assert "downscale of the region is empty" in refused_by_settings((2, 2), dict(block_size=2, filter_scaling=8.0))      # rint(2 / 8) = 0

    assert call() == 0
    ctx.sync()
    assert_outputs(outs, e["want"], "after the refusals")
    assert all(p.unchanged() for p in ins)
    assert tuple(region) == e["info"]["region"] == f.filter_region() and tap_equals(f, e["info"])
    f.close()


def test_refusal_messages_are_those_of_apply(ctx):
    import torch
    import livevisionkit_amd as lvk
    f = lvk.DeblockingFilter(ctx)
    for conf, (rows, cols) in [(dict(), (14, 200)), (dict(filter_size=257), (48, 86)), (dict(block_size=2, filter_scaling=8.0), (2, 2))]:
        f.configure(**conf)
        with pytest.raises(lvk.LvkHipError) as err:
            f.apply(torch.from_numpy(blocky(rows, cols, seed=1)).cuda(), nd.FMT_YUV)
        packed = str(err.value).replace("lvk_hip_deblock_apply", "ENTRY")
        for fmt, shape in (("UYVY", (rows, cols, 2)), ("BGR3", (rows, cols, 3)), ("Y800", (rows, cols))):
            with pytest.raises(lvk.LvkHipError) as err:
                f.apply_obs(fmt, [torch.zeros(shape, dtype=torch.uint8, device="cuda")])
            assert str(err.value).replace("lvk_hip_deblock_apply_obs", "ENTRY") == packed, (fmt, conf)
    f.close()


def test_two_filters_on_one_context(ctx):
    ca, cb = C_TABLES, (34, 50, 2, 8, 7, 2.5)
    ea, eb = expected("YUY2", ca), expected("AYUV", cb)
    a, b = new_filter(ctx, ca), new_filter(ctx, cb)
    pa, pb = [gpu(p) for p in ea["planes"]], [gpu(p) for p in eb["planes"]]
    for _ in range(2):
        ga, ra = a.apply_obs("YUY2", pa)
        gb, rb = b.apply_obs("AYUV", pb)
        ctx.sync()
        assert ra == ea["info"]["region"] and rb == eb["info"]["region"]
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(ga, ea["want"]))
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(gb, eb["want"]))
        assert tap_equals(a, ea["info"]) and tap_equals(b, eb["info"])
    a.close(); b.close()


def test_the_python_methods_forms(ctx):
    import torch
    import livevisionkit_amd as lvk
    for fmt, case in (("UYVY", CASES_EVEN[5]), ("I422", CASES_EVEN[6]), ("Y800", CASES_ODD[2]), ("NV12", CASES_420[6]), ("BGRA", CASES_ODD[3])):
        e = expected(fmt, case)
        f = new_filter(ctx, case)
        planes = [gpu(p) for p in e["planes"]]
        by_name, r1 = f.apply_obs(fmt, planes)
        by_number, r2 = f.apply_obs(ctx.VIDEO_FORMATS[fmt], tuple(planes))
        given = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
        back, r3 = f.apply_obs(fmt, planes, out=given)
        ctx.sync()
        assert r1 == r2 == r3 == e["info"]["region"]
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
        f.close()
