"""lvk_hip_remap_map_obs and lvk_hip_lens_apply_obs on the MI355X (csrc/remap_obs.hip, csrc/lens_filter.hip), bit for bit against
the specification of tests/lens_obs_cases.py (whose liveness tests/test_lens_obs_spec.py asserts) and against the GPU's own chains.  Every plane is a
view into a buffer of guard bytes: pitch padding, what lies before and behind a plane, and the bytes lvk_hip_egress_obs leaves alone (the last quarter of
an RGBA / BGRA / BGRX plane) must come back unchanged, and so must the input planes, in test mode too."""
import ctypes

import numpy as np
import pytest

from tests import lens_420_cases as c420
from tests.lens_obs_cases import (BG, DIRECT4, F420, F422, FILTER_PROFILES, FORMATS, FUSABLE, GUARD, PRIM_CASES, TEXTURES, case_id, filter_expected,
                                  filter_sizes, maps_of, params_of, prim_expected, prim_textures, profile_id, size_id)

pytestmark = pytest.mark.gpu

ERR_ARG = -1
FORMAT_BGR, FORMAT_YUV = 0, 4
_P, _I = ctypes.c_void_p, ctypes.c_int


def gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Buf:
    """An array [rows, ...] on the GPU as a view `offset` bytes into a buffer of guard bytes (`fill`, or random bytes), rows `pad` bytes longer than their
    pixels."""

    def __init__(self, arr, pad=0, offset=0, fill=None, seed=0):
        import torch
        self.shape = tuple(arr.shape)
        self.row = int(np.prod(self.shape[1:]))
        self.pitch, self.offset = self.row + pad, offset
        inner = [int(np.prod(self.shape[i + 1:])) for i in range(1, len(self.shape))]
        self.strides = (self.pitch, *inner)
        n = offset + self.shape[0] * self.pitch + 16
        self.flat = np.full(n, fill, np.uint8) if fill is not None else np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
        if fill is None:
            self.host(self.flat)[...] = arr
        self.buf = torch.from_numpy(self.flat).cuda()
        self.view = self.buf.as_strided(self.shape, self.strides, offset)

    def host(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.offset:], shape=self.shape, strides=self.strides)

    def expect(self, want):
        out = self.flat.copy()
        self.host(out)[...] = want
        return out

    def unchanged(self):
        return np.array_equal(self.buf.cpu().numpy(), self.flat)


def placement(fmt, pads, offsets):
    """The 4-byte DirectIngest planes are tight (steps[0] == 4 * cols); an AYUV plane that leaves through lvk_hip_egress_obs starts on a dword."""
    if fmt in DIRECT4:
        return (0, 0, 0), offsets
    if fmt == "AYUV":
        return tuple(4 * p for p in pads), tuple(4 * o for o in offsets)
    return pads, offsets


def guarded_outputs(want, pads=(0, 0, 0), offsets=(0, 0, 0)):
    return [Buf(w, pads[i], offsets[i], fill=GUARD) for i, w in enumerate(want)]


def assert_outputs(outs, want, what):
    for i, (p, w) in enumerate(zip(outs, want)):
        got, exp = p.buf.cpu().numpy(), p.expect(w)
        assert np.array_equal(got, exp), "%s: output plane %d: %d bytes differ" % (what, i, int((got != exp).sum()))


# ---- the primitive ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PRIM_CASES, ids=case_id)
def test_remap_map_obs_bit_exact(ctx, case):
    fmt, size = case
    for kind in prim_textures(size):
        for name in maps_of(size):
            e = prim_expected(fmt, size, name, kind)
            outs = guarded_outputs(e["want"])
            src, m = gpu(e["src"]), gpu(e["map"])
            views = [p.view for p in outs]
            assert ctx.remap_map_obs(fmt, src, m, views, bg=BG) is views
            ctx.sync()
            assert_outputs(outs, e["want"], "%s %s" % (name, kind))
            assert np.array_equal(src.cpu().numpy(), e["src"])


@pytest.mark.parametrize("precision", ["exact", "1lsb"])
@pytest.mark.parametrize("case", PRIM_CASES, ids=case_id)
def test_remap_map_obs_equals_the_gpus_own_chain(ctx, case, precision):
    import torch
    import livevisionkit_amd as lvk
    fmt, size = case
    ctx.set_remap_precision(lvk.REMAP_1LSB if precision == "1lsb" else lvk.REMAP_EXACT)
    try:
        for name in maps_of(size):
            e = prim_expected(fmt, size, name, "smooth")
            src, m = gpu(e["src"]), gpu(e["map"])
            got = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
            chained = [torch.full(w.shape, GUARD, dtype=torch.uint8, device="cuda") for w in e["want"]]
            ctx.remap_map_obs(fmt, src, m, got, bg=BG)
            ctx.egress_obs(fmt, ctx.remap_map(src, m, bg=BG, yuv=True), chained)
            ctx.sync()
            for i, (g, c, w) in enumerate(zip(got, chained, e["want"])):
                assert torch.equal(g, c), (name, i)
                d = np.abs(g.cpu().numpy().astype(np.int16) - w)
                assert int(d.max()) <= (1 if precision == "1lsb" else 0), (name, i, int(d.max()))
    finally:
        ctx.set_remap_precision(lvk.REMAP_EXACT)


# Pitches + 0 / + 1 / + 13; the plane bases 0 .. 3 bytes off a dword (the byte-store branches of every sink); odd and even chroma offsets
ALIGNMENTS = [((0, 0, 0), (1, 0, 0)), ((1, 1, 1), (2, 1, 1)), ((13, 13, 1), (3, 1, 2)), ((0, 13, 13), (0, 1, 1)), ((1, 0, 13), (2, 2, 3))]


@pytest.mark.parametrize("align", ALIGNMENTS, ids=lambda a: "pad%d.%d.%d-off%d.%d.%d" % (a[0] + a[1]))
@pytest.mark.parametrize("size", [(66, 254), (67, 258)], ids=size_id)
@pytest.mark.parametrize("fmt", FUSABLE)
def test_padded_pitches_and_offsets_keep_their_guard_bytes(ctx, fmt, size, align):
    import torch
    pads, offsets = align
    rows, cols = size
    for name in ("near", "far"):
        e = prim_expected(fmt, size, name, "random")
        outs = guarded_outputs(e["want"], pads, offsets)
        # the inputs padded as well: a source pitch that is no multiple of 4, a map pitch that is a multiple of 8
        src = torch.zeros((rows, 3 * cols + pads[0]), dtype=torch.uint8, device="cuda")
        src[:, :3 * cols] = gpu(e["src"]).reshape(rows, 3 * cols)
        m = torch.zeros((rows, cols + pads[1], 2), dtype=torch.float32, device="cuda")
        m[:, :cols] = gpu(e["map"])
        ctx.remap_map_obs(fmt, src[:, :3 * cols].unflatten(1, (cols, 3)), m[:, :cols], [p.view for p in outs], bg=BG)
        ctx.sync()
        assert_outputs(outs, e["want"], name)


def test_the_420_formats_go_through_the_420_primitive(ctx):
    size = (34, 130)
    e = c420.prim_expected(size, "near", "random")
    for fmt, lay in (("I420", tuple), ("I40A", tuple), ("NV12", c420.as_nv12)):
        want = lay(e["want"])
        outs = guarded_outputs(want, (1, 1, 1), (1, 1, 1))
        ctx.remap_map_obs(fmt, gpu(e["src"]), gpu(e["map"]), [p.view for p in outs], bg=c420.BG)
        ctx.sync()
        assert_outputs(outs, want, fmt)


def raw_fn(ctx, name, argtypes):
    """The entry with plain pointers where _native.py binds arrays: a NULL array can be passed."""
    return ctypes.CFUNCTYPE(_I, *argtypes)(ctypes.cast(getattr(ctx.lib, name), _P).value)


def arr3(vals, ctype):
    return (ctype * 3)(*(list(vals) + [None if ctype is _P else 0] * (3 - len(vals))))


@pytest.mark.parametrize("fmt", ["I422", "UYVY", "I444", "AYUV"])
def test_refused_primitive_calls_change_nothing(ctx, fmt):
    size = (16, 34)
    rows, cols = size
    vf = ctx.VIDEO_FORMATS[fmt]
    e = prim_expected(fmt, size, "near", "random")
    outs = guarded_outputs(e["want"], (4, 4, 4))
    n = len(outs)
    src, m = gpu(e["src"]), gpu(e["map"])
    bg = (ctypes.c_uint8 * 3)(*BG)
    sp, mp, ss, ms = src.data_ptr(), m.data_ptr(), 3 * cols, 8 * cols
    op, st = [p.view.data_ptr() for p in outs], [p.pitch for p in outs]
    rowb = [p.row for p in outs]
    fn = raw_fn(ctx, "lvk_hip_remap_map_obs", [_P, _I, _P, _I, _I, _I, _P, _P, _P, _I, _P])

    def call(vf=vf, sp=sp, ss=ss, size=size, op=op, st=st, mp=mp, ms=ms, bg=bg, null_planes=False, null_steps=False):
        return fn(ctx.handle, vf, sp, ss, size[0], size[1], None if null_planes else arr3(op, _P), None if null_steps else arr3(st, _I), mp, ms, bg)

    def unchanged():
        ctx.sync()
        return all(p.unchanged() for p in outs) and np.array_equal(src.cpu().numpy(), e["src"])

    refused = [dict(sp=None), dict(mp=None), dict(bg=None), dict(null_planes=True), dict(null_steps=True), dict(ss=ss - 1),
               dict(ms=ms - 8), dict(ms=ms + 4), dict(mp=mp + 4), dict(size=(0, cols)), dict(size=(rows, 0)), dict(size=(-2, cols))]
    refused += [dict(vf=v) for v in (0, 17, -1, 99, ctx.VIDEO_FORMATS["BGR3"], ctx.VIDEO_FORMATS["Y800"], ctx.VIDEO_FORMATS["RGBA"], ctx.VIDEO_FORMATS["BGRA"],
                                    ctx.VIDEO_FORMATS["BGRX"])]
    if fmt in F422:
        refused.append(dict(size=(rows, cols - 1)))
    for i in range(n):
        refused.append(dict(op=op[:i] + [None] + op[i + 1:]))                       # a NULL plane that is in use
        refused.append(dict(st=st[:i] + [rowb[i] - 1] + st[i + 1:]))                # a pitch below its row
        refused.append(dict(st=st[:i] + [1 << 24] + st[i + 1:]))                    # a pitch the sinks' 24-bit factors cannot hold
        refused.append(dict(op=op[:i] + [sp + 5] + op[i + 1:]))                     # on the source, inside the map
        refused.append(dict(op=op[:i] + [mp + ms * (rows - 1) + 8 * cols - 1] + op[i + 1:]))
    if n == 3:
        refused.append(dict(op=[op[0], op[0] + st[0] * (rows - 1), op[2]]))         # two outputs on each other
        refused.append(dict(op=[op[0], op[1], op[1] + 1]))
    for a in refused:
        assert call(**a) == ERR_ARG, a
        assert unchanged(), a
    assert call() == 0
    ctx.sync()
    assert_outputs(outs, e["want"], "after the refusals")


# ---- the filter on planes ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def lc(ctx):
    import livevisionkit_amd as lvk
    made = []

    def make(profile=None, test_mode=False):
        made.append(lvk.LCFilter(profile, test_mode, context=ctx))
        return made[-1]
    yield make
    ctx.sync()
    for f in made:
        f.close()


def apply_guarded(ctx, f, fmt, e, what, pads=(0, 0, 0), offsets=(0, 0, 0)):
    pads, offsets = placement(fmt, pads, offsets)
    ins = [Buf(p, pads[i], offsets[i], seed=10 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], pads, offsets)
    views = [p.view for p in outs]
    assert f.apply_obs(fmt, [p.view for p in ins], out=views) == views
    ctx.sync()
    for i, p in enumerate(ins):
        assert p.unchanged(), "%s: input plane %d changed" % (what, i)
    assert_outputs(outs, e["want"], what)


FILTER_PARAMS = [(f, s, p) for f in FORMATS for s in filter_sizes(f) for p in FILTER_PROFILES]


@pytest.mark.parametrize("fmt,size,profile", FILTER_PARAMS, ids=lambda v: v if isinstance(v, str) else size_id(v) if isinstance(v, tuple) else profile_id(v))
def test_apply_obs_bit_exact(ctx, lc, fmt, size, profile):
    f = lc(params_of(profile, *size), False)
    for test_mode in (False, True):
        if test_mode and fmt == "Y800":
            continue                                               # a refusal: test_refused_filter_calls_change_nothing
        f.configure(params_of(profile, *size), test_mode)
        for k, kind in enumerate(TEXTURES):
            e = filter_expected(fmt, size, profile, test_mode, kind)
            apply_guarded(ctx, f, fmt, e, "%s %s" % ("grid" if test_mode else "plain", kind), pads=(k, 13 * k, k), offsets=(k, k, 3 * k))
            assert f.view(*size) == e["view"]


def run_obs(ctx, f, fmt, planes):
    out = f.apply_obs(fmt, [gpu(p) for p in planes])
    ctx.sync()
    return [o.cpu().numpy() for o in out]


def written(fmt, got, want):
    """A freshly allocated output holds anything where the egress writes nothing: compared where `want` is not the guard pattern's untouched tail."""
    if fmt not in DIRECT4:
        return all(np.array_equal(g, w) for g, w in zip(got, want))
    n = want[0].size * 3 // 4
    return np.array_equal(got[0].reshape(-1)[:n], want[0].reshape(-1)[:n])


def test_one_handle_alternates_formats_sizes_and_entries(ctx, lc):
    big, small = (66, 258), (16, 34)
    f = lc(params_of(0, *big), False)
    steps = 0
    for fmt, size in [("UYVY", big), ("I444", small), ("packed", big), ("RGBA", small), ("I420", big), ("420", small), ("Y800", big), ("AYUV", big),
                      ("BGR3", small), ("gray", small), ("I42A", big), ("NV12", small), ("YVYU", big)]:
        if fmt == "packed":
            e = c420.packed_expected(size, 0, False, True)
            got = f.apply(gpu(e["src"]), FORMAT_YUV)
            ctx.sync()
            assert np.array_equal(got.cpu().numpy(), e["want"])
        elif fmt == "420":
            e = c420.filter_expected(size, 0, False, "smooth", at=big)
            got = f.apply_yuv420(*[gpu(p) for p in e["planes"]])
            ctx.sync()
            assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, e["want"]))
        elif fmt == "gray":
            g = c420.packed_source(*size, "smooth")[..., 0]
            want = c420.oracle().remap_map(np.stack([g, g, g], axis=2), c420.lens_map(0, *size, at=big)[0], bg=(0, 0, 0), yuv=False)[..., 0]
            got = f.apply(gpu(g))
            ctx.sync()
            assert np.array_equal(got.cpu().numpy(), want)
        else:
            # one camera: the profile's parameters are those of the big frame at either size
            e = filter_expected(fmt, size, 0, False, "smooth", at=big)
            assert written(fmt, run_obs(ctx, f, fmt, e["planes"]), e["want"]), (fmt, size)
        steps += 1
    assert steps == 13


def test_a_configure_between_two_calls_and_two_filters_on_one_context(ctx, lc):
    size = (66, 258)
    f, g = lc(params_of(0, *size), False), lc(params_of(1, *size), True)
    for fmt in ("UYVY", "I444", "BGRA"):
        f.configure(params_of(0, *size), False)
        a = filter_expected(fmt, size, 0, False, "smooth")
        b = filter_expected(fmt, size, 1, True, "smooth")
        assert written(fmt, run_obs(ctx, f, fmt, a["planes"]), a["want"])
        assert written(fmt, run_obs(ctx, g, fmt, b["planes"]), b["want"])
        f.configure(params_of(3, *size), True)                     # another profile and the grid, same size: the map is rebuilt
        c = filter_expected(fmt, size, 3, True, "smooth")
        assert written(fmt, run_obs(ctx, f, fmt, c["planes"]), c["want"])
        assert written(fmt, run_obs(ctx, g, fmt, b["planes"]), b["want"])
        f.configure(None, False)
        d = filter_expected(fmt, size, None, False, "smooth")
        assert written(fmt, run_obs(ctx, f, fmt, d["planes"]), d["want"])
        assert not written(fmt, [w for w in d["want"]], a["want"])


@pytest.mark.parametrize("fmt", ["UYVY", "I444", "BGRA"])
def test_steady_state_allocates_nothing(ctx, lc, fmt):
    """As tests/test_lens_420_gpu.py taps it: the pool is emptied and given ONE block of the packed frame's size, filled with a pattern.  Every call must
    take that block and give it back: afterwards lvk_hip_malloc of the size hands out the same address, and the block holds the packed frame the call made
    in it (the ingest with the grid) -- a call that allocated memory of its own would leave the pattern.  Three calls in a row."""
    size = (270, 480)
    rows, cols = size
    e = filter_expected(fmt, size, 0, True, "smooth")
    o = c420.oracle()
    gridded = o.draw_grid(o.ingest_obs(fmt, list(e["planes"])), c420.GRID, c420.MAGENTA_YUV if fmt != "BGRA" else c420.MAGENTA_BGR, 1)
    f = lc(params_of(0, *size), True)
    planes = [gpu(p) for p in e["planes"]]
    nbytes = ((3 * cols + 3) & ~3) * rows
    assert nbytes == gridded.size
    L = ctx.lib
    ctx.sync()
    assert L.lvk_hip_trim(ctx.handle) == 0
    block = ctypes.c_void_p()
    assert L.lvk_hip_malloc(ctx.handle, nbytes, ctypes.byref(block)) == 0
    pattern = np.full(nbytes, GUARD, np.uint8)
    for _ in range(3):
        assert L.lvk_hip_upload(ctx.handle, block, pattern.ctypes.data_as(ctypes.c_void_p), nbytes) == 0
        ctx.sync()
        assert L.lvk_hip_free(ctx.handle, block) == 0
        got = run_obs(ctx, f, fmt, e["planes"])
        again = ctypes.c_void_p()
        assert L.lvk_hip_malloc(ctx.handle, nbytes, ctypes.byref(again)) == 0
        assert again.value == block.value
        held = np.zeros(nbytes, np.uint8)
        assert L.lvk_hip_download(ctx.handle, held.ctypes.data_as(ctypes.c_void_p), again, nbytes) == 0
        ctx.sync()
        assert np.array_equal(held.reshape(gridded.shape), gridded)
        assert written(fmt, got, e["want"])
    assert L.lvk_hip_free(ctx.handle, block) == 0
    del planes


@pytest.mark.parametrize("fmt", ["I422", "YUY2", "I444", "AYUV", "BGR3", "RGBA", "Y800", "I420", "NV12"])
def test_refused_filter_calls_change_nothing(ctx, lc, fmt):
    import livevisionkit_amd as lvk
    size = (16, 34)
    rows, cols = size
    vf = ctx.VIDEO_FORMATS[fmt]
    grid = fmt != "Y800"
    e = filter_expected(fmt, size, 0, grid, "random")
    f = lc(params_of(0, *size), grid)
    pad = 0 if fmt in DIRECT4 else 4
    ins = [Buf(p, pad, 0, seed=20 + i) for i, p in enumerate(e["planes"])]
    outs = guarded_outputs(e["want"], (pad,) * 3)
    n = len(ins)
    ip, isteps = [p.view.data_ptr() for p in ins], [p.pitch for p in ins]
    op, osteps = [p.view.data_ptr() for p in outs], [p.pitch for p in outs]
    rowb = [p.row for p in ins]
    prows = [p.shape[0] for p in ins]
    fn = raw_fn(ctx, "lvk_hip_lens_apply_obs", [_P, _I, _P, _P, _P, _P, _I, _I])

    def call(handle=f.handle, vf=vf, ip=ip, isteps=isteps, op=op, osteps=osteps, size=size, null=()):
        a = [None if "ip" in null else arr3(ip, _P), None if "isteps" in null else arr3(isteps, _I),
             None if "op" in null else arr3(op, _P), None if "osteps" in null else arr3(osteps, _I)]
        return fn(handle, vf, a[0], a[1], a[2], a[3], size[0], size[1])

    def unchanged():
        ctx.sync()
        return all(p.unchanged() for p in outs) and all(p.unchanged() for p in ins)

    refused = [dict(handle=None), dict(null=("ip",)), dict(null=("isteps",)), dict(null=("op",)), dict(null=("osteps",))]
    refused += [dict(vf=v) for v in (0, 17, -1, 99)]                                # an unknown format
    refused += [dict(size=s) for s in [(0, cols), (rows, 0), (-2, cols), (rows, -2), (1, cols), (rows, 1)]]      # below 2 with a profile selected
    if fmt in F422 or fmt in F420:
        refused += [dict(size=(rows, cols - 1)), dict(size=(rows, 15))]             # odd cols
    if fmt in F420:
        refused += [dict(size=(rows - 1, cols)), dict(size=(15, cols))]             # odd rows
    for i in range(n):
        refused.append(dict(ip=ip[:i] + [None] + ip[i + 1:]))                       # a NULL plane that is in use
        refused.append(dict(op=op[:i] + [None] + op[i + 1:]))
        refused.append(dict(isteps=isteps[:i] + [rowb[i] - 1] + isteps[i + 1:]))    # a pitch below its row
        refused.append(dict(osteps=osteps[:i] + [rowb[i] - 1] + osteps[i + 1:]))
        refused.append(dict(osteps=osteps[:i] + [1 << 24] + osteps[i + 1:]))        # a plane the kernels' 32-bit offsets cannot address
        refused.append(dict(op=op[:i] + [ip[0]] + op[i + 1:]))                      # in place, and ending inside an input plane
        refused.append(dict(op=op[:i] + [ip[n - 1] + isteps[n - 1] * (prows[n - 1] - 1) + rowb[n - 1] - 1] + op[i + 1:]))
    if fmt in DIRECT4:
        refused += [dict(isteps=[4 * cols + 4]), dict(osteps=[4 * cols + 4]), dict(isteps=[4 * cols - 4]), dict(osteps=[4 * cols - 4])]
    if n == 3:
        refused.append(dict(op=[op[0], op[0] + osteps[0] * (rows - 1), op[2]]))     # two outputs on each other
        refused.append(dict(op=[op[0], op[1], op[1] + 1]))
    if n == 2:
        refused.append(dict(op=[op[0], op[0] + osteps[0] * (rows - 1)]))
    for a in refused:
        assert call(**a) == ERR_ARG, a
        assert unchanged(), a
    if fmt == "Y800":
        f.configure(params_of(0, *size), True)                                     # the grid kernel writes three bytes per pixel
        assert call() == ERR_ARG and unchanged()
        with pytest.raises(lvk.LvkHipError):
            f.apply_obs(fmt, [p.view for p in ins], out=[p.view for p in outs])
        assert unchanged()
        f.configure(params_of(0, *size), False)
    if fmt == "AYUV":
        # the one refusal of the chain the fused kernel has not: without a profile the frame leaves through lvk_hip_egress_obs, in dwords
        f.configure(None, grid)
        assert call(op=[op[0] + 1]) == ERR_ARG and call(osteps=[osteps[0] + 2]) == ERR_ARG and unchanged()
        f.configure(params_of(0, *size), grid)
    assert call() == 0
    ctx.sync()
    assert_outputs(outs, e["want"], "after the refusals")
    assert all(p.unchanged() for p in ins)


def test_the_python_methods_forms(ctx, lc):
    import torch
    size = (16, 34)
    f = lc(params_of(1, *size), False)
    for fmt in ("UYVY", "I422", "Y800", "NV12"):
        e = filter_expected(fmt, size, 1, False, "smooth")
        planes = [gpu(p) for p in e["planes"]]
        assert [tuple(p.shape) for p in planes] == [tuple(s) for s in f.obs_plane_shapes(fmt, *size)]
        by_name, by_number = f.apply_obs(fmt, planes), f.apply_obs(ctx.VIDEO_FORMATS[fmt], planes)
        given = [torch.zeros_like(p) for p in planes]
        back = f.apply_obs(fmt, tuple(planes), out=given)
        ctx.sync()
        assert isinstance(by_name, list) and all(b is g for b, g in zip(back, given))
        for a, b, c, w in zip(by_name, by_number, given, e["want"]):
            assert a.shape == w.shape and np.array_equal(a.cpu().numpy(), w) and torch.equal(a, b) and torch.equal(a, c)
        with pytest.raises(ValueError):
            f.apply_obs(fmt, planes, out=given[:-1] if len(given) > 1 else given + given)
    e = prim_expected("I444", size, "near", "smooth")
    planes = [torch.zeros(w.shape, dtype=torch.uint8, device="cuda") for w in e["want"]]
    assert ctx.remap_map_obs(ctx.VIDEO_FORMATS["I444"], gpu(e["src"]), gpu(e["map"]), planes, bg=BG) is planes
    ctx.sync()
    assert all(np.array_equal(p.cpu().numpy(), w) for p, w in zip(planes, e["want"]))
