"""lvk_hip_remap_map_yuv420 and the lens filter object on the MI355X (csrc/lens_filter.hip), bit for bit against the specification
of tests/lens_420_cases.py (whose liveness tests/test_lens_420_spec.py asserts) and against the GPU's own chains.  Output planes are views into buffers
of guard bytes (the Plane of tests/test_deblock_420_gpu.py): the pitch padding and what lies before and behind a plane must come back unchanged."""
import ctypes

import numpy as np
import pytest

from tests.lens_420_cases import (BG, FILTER_PROFILES, FILTER_SIZES, PRIM_SIZES, TEXTURES, filter_expected, layout_of, lens_map, maps_of, oracle,
                                  packed_expected, packed_source, params_of, prim_expected, prim_texture, profile_id, size_id)
from tests.test_deblock_420_gpu import Plane

pytestmark = pytest.mark.gpu

ERR_ARG = -1
LAYOUTS = ["i420", "nv12"]
FORMAT_BGR, FORMAT_BGRA, FORMAT_YUV = 0, 1, 4


def gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded_outputs(want, pads=(0, 0, 0), offsets=(0, 0, 0)):
    return [Plane(w, pads[i], offsets[i], fill=0x5A) for i, w in enumerate(want)]


def assert_outputs(outs, want, what):
    for i, (p, w) in enumerate(zip(outs, want)):
        got, exp = p.buf.cpu().numpy(), p.expect(w)
        assert np.array_equal(got, exp), "%s: output plane %d: %d bytes differ" % (what, i, int((got != exp).sum()))


# ---- the primitive ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", PRIM_SIZES, ids=size_id)
def test_remap_map_yuv420_bit_exact(ctx, size, layout):
    for kind in prim_texture(size):
        for name in maps_of(size):
            e = prim_expected(size, name, kind)
            want = layout_of(e["want"], layout)
            outs = guarded_outputs(want)
            src, m = gpu(e["src"]), gpu(e["map"])
            ctx.remap_map_yuv420(src, m, bg=BG, nv12=layout == "nv12", out=[p.view for p in outs])
            ctx.sync()
            assert_outputs(outs, want, "%s %s" % (name, kind))
            assert np.array_equal(src.cpu().numpy(), e["src"])


# Pitches + 0 / + 1 / + 13, the luma base 1, 2 and 3 bytes off a dword (the byte-store path), the NV12 UV and the I420 chroma bases off by 1
ALIGNMENTS = [((0, 0, 0), (1, 0, 0)), ((1, 1, 1), (2, 1, 1)), ((13, 13, 1), (3, 1, 2)), ((0, 13, 13), (0, 1, 1)), ((1, 0, 13), (2, 0, 1))]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("align", ALIGNMENTS, ids=lambda a: "pad%d.%d.%d-off%d.%d.%d" % (a[0] + a[1]))
@pytest.mark.parametrize("size", [(14, 18), (16, 34), (66, 258)], ids=size_id)
def test_padded_pitches_and_offsets_keep_their_guard_bytes(ctx, size, align, layout):
    pads, offsets = align
    for name in ("near", "far"):
        e = prim_expected(size, name, "random")
        want = layout_of(e["want"], layout)
        outs = guarded_outputs(want, pads, offsets)
        ctx.remap_map_yuv420(gpu(e["src"]), gpu(e["map"]), bg=BG, nv12=layout == "nv12", out=[p.view for p in outs])
        ctx.sync()
        assert_outputs(outs, want, name)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_padded_source_and_map(ctx, layout):
    # a source pitch that is no multiple of 4 and a map with a padded pitch (a multiple of 8)
    import torch
    size = (18, 66)
    rows, cols = size
    e = prim_expected(size, "near", "random")
    src = torch.zeros((rows, 3 * cols + 5), dtype=torch.uint8, device="cuda")
    src[:, :3 * cols] = gpu(e["src"]).reshape(rows, 3 * cols)
    m = torch.zeros((rows, cols + 3, 2), dtype=torch.float32, device="cuda")
    m[:, :cols] = gpu(e["map"])
    want = layout_of(e["want"], layout)
    outs = guarded_outputs(want)
    ctx.remap_map_yuv420(src[:, :3 * cols].unflatten(1, (cols, 3)), m[:, :cols], bg=BG, nv12=layout == "nv12", out=[p.view for p in outs])
    ctx.sync()
    assert_outputs(outs, want, "padded")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", [(16, 34), (66, 258), (270, 480)], ids=size_id)
def test_one_lsb_mode_equals_the_gpus_own_chain(ctx, size, layout):
    import torch
    import livevisionkit_amd as lvk
    nv12 = layout == "nv12"
    e = prim_expected(size, "lens", "smooth")
    src, m = gpu(e["src"]), gpu(e["map"])
    ctx.set_remap_precision(lvk.REMAP_1LSB)
    try:
        got = ctx.remap_map_yuv420(src, m, bg=BG, nv12=nv12)
        packed = ctx.remap_map(src, m, bg=BG, yuv=True)
        chained = ctx.egress_yuv420(packed, nv12=nv12)
        ctx.sync()
    finally:
        ctx.set_remap_precision(lvk.REMAP_EXACT)
    for i, (g, c) in enumerate(zip(got, chained)):
        assert torch.equal(g, c), i
    exact = ctx.remap_map_yuv420(src, m, bg=BG, nv12=nv12)
    ctx.sync()
    for g, w in zip(exact, layout_of(e["want"], layout)):
        assert np.array_equal(g.cpu().numpy(), w)
    if size[0] >= 270:
        # the mode is live there: the regrouped weights change a few bytes of the packed frame (5 in tests/np_easu_1lsb.py's arithmetic, none at the
        # two smaller sizes), each by 1
        d = packed.cpu().numpy().astype(np.int16) - e["remapped"]
        assert d.any() and int(np.abs(d).max()) == 1


def raw_prim(ctx, src, src_step, size, outs, steps, nv12, m, map_step, bg):
    return ctx.lib.lvk_hip_remap_map_yuv420(ctx.handle, src, src_step, size[0], size[1], outs[0], steps[0], outs[1], steps[1], outs[2], steps[2], nv12, m, map_step, bg)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_refused_primitive_calls_change_nothing(ctx, layout):
    size = (16, 34)
    rows, cols = size
    nv12 = 1 if layout == "nv12" else 0
    e = prim_expected(size, "near", "random")
    want = layout_of(e["want"], layout)
    outs = guarded_outputs(want, (4, 4, 4))
    n = len(outs)
    src, m = gpu(e["src"]), gpu(e["map"])
    bg =(ctypes.c_uint8 * 3)(*BG)
    sp, mp, ss, ms = src.data_ptr(), m.data_ptr(), 3 * cols, 8 * cols
    op = [p.view.data_ptr() for p in outs] + [None] * (3 - n)
    st = [p.pitch for p in outs] + [0] * (3 - n)
    before = [p.buf.cpu().numpy() for p in outs]

    def unchanged():
        ctx.sync()
        return (all(np.array_equal(p.buf.cpu().numpy(), b) for p, b in zip(outs, before)) and np.array_equal(src.cpu().numpy(), e["src"])
                and np.array_equal(m.cpu().numpy().view(np.uint32), e["map"].view(np.uint32)))

    refused = []                                                   # (src, src step, size, outs, out steps, map, map step, bg)
    refused.append((None, ss, size, op, st, mp, ms, bg))           # NULL pointers in use
    refused.append((sp, ss, size, op, st, None, ms, bg))
    refused.append((sp, ss, size, op, st, mp, ms, None))
    for i in range(n):
        refused.append((sp, ss, size, op[:i] + [None] + op[i + 1:], st, mp, ms, bg))
    for bad in [1, 0, -2, 3, 15]:                                  # odd sizes and sizes below 2
        refused.append((sp, ss, (bad, cols), op, st, mp, ms, bg))
        refused.append((sp, ss, (rows, bad), op, st, mp, ms, bg))
    refused.append((sp, ss - 1, size, op, st, mp, ms, bg))          # pitches below their rows
    row = [cols, cols if nv12 else cols // 2, cols // 2]
    for i in range(n):
        s = list(st); s[i] = row[i] - 1
        refused.append((sp, ss, size, op, s, mp, ms, bg))
    refused.append((sp, ss, size, op, st, mp, ms - 8, bg))          # the map: a short pitch, a pitch or a base that is no multiple of 8
    refused.append((sp, ss, size, op, st, mp, ms + 4, bg))
    refused.append((sp, ss, size, op, st, mp + 4, ms, bg))
    # overlaps: an output plane on the source, inside the map, two outputs on each other
    refused.append((sp, ss, size, [sp + 5] + op[1:], st, mp, ms, bg))
    refused.append((sp, ss, size, [op[0], sp + ss * (rows - 1)] + op[2:], st, mp, ms, bg))
    refused.append((sp, ss, size, [mp + 16] + op[1:], st, mp, ms, bg))
    refused.append((sp, ss, size, [op[0], mp + ms * (rows - 1) + 8 * cols - 1] + op[2:], st, mp, ms, bg))
    refused.append((sp, ss, size, [op[0], op[0] + st[0] * (rows - 1)] + op[2:], st, mp, ms, bg))
    if not nv12:
        refused.append((sp, ss, size, [op[0], op[1], op[1] + 1], st, mp, ms, bg))
    for a in refused:
        assert raw_prim(ctx, a[0], a[1], a[2], a[3], a[4], nv12, a[5], a[6], a[7]) == ERR_ARG, a
        assert unchanged(), a
    assert raw_prim(ctx, sp, ss, size, op[:2] + [sp] if nv12 else op, st, nv12, mp, ms, bg) == 0        # NV12 ignores o_v, whatever it is
    ctx.sync()
    assert_outputs(outs, want, "after the refusals")


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


def apply_guarded(ctx, f, e, layout, what, pads=(0, 0, 0), offsets=(0, 0, 0)):
    planes, want = layout_of(e["planes"], layout), layout_of(e["want"], layout)
    ins = [Plane(p, pads[i], offsets[i], seed=10 + i) for i, p in enumerate(planes)]
    outs = guarded_outputs(want, pads, offsets)
    f.apply_yuv420(*[p.view for p in ins], out=[p.view for p in outs])
    ctx.sync()
    for i, p in enumerate(ins):
        assert np.array_equal(p.buf.cpu().numpy(), p.flat), "%s: input plane %d changed" % (what, i)
    assert_outputs(outs, want, what)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("test_mode", [False, True], ids=["plain", "grid"])
@pytest.mark.parametrize("profile", FILTER_PROFILES, ids=profile_id)
@pytest.mark.parametrize("size", FILTER_SIZES, ids=size_id)
def test_apply_yuv420_bit_exact(ctx, lc, size, profile, test_mode, layout):
    f = lc(params_of(profile, *size), test_mode)
    for k, kind in enumerate(TEXTURES):
        e = filter_expected(size, profile, test_mode, kind)
        apply_guarded(ctx, f, e, layout, kind, pads=(k, 13 * k, k), offsets=(k, k, 3 * k))
        assert f.view(*size) == e["view"]


def fresh_planes(ctx, lc, params, test_mode, planes, layout):
    f = lc(params, test_mode)
    out = f.apply_yuv420(*[gpu(p) for p in layout_of(planes, layout)])
    ctx.sync()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_object_follows_sizes_and_profiles(ctx, lc, layout):
    import livevisionkit_amd as lvk
    big, small = (66, 130), (34, 66)
    f = lc(params_of(0, *big), False)
    steps = []                                                  # (size, profile, test mode)

    def step(size, profile, test_mode, what):
        # one camera: the profile's parameters are those of the big frame at either size
        e = filter_expected(size, profile, test_mode, "smooth", at=big)
        got = f.apply_yuv420(*[gpu(p) for p in layout_of(e["planes"], layout)])
        ctx.sync()
        want = layout_of(e["want"], layout)
        fresh = fresh_planes(ctx, lc, params_of(profile, *big), test_mode, e["planes"], layout)
        for i, (g, w, fr) in enumerate(zip(got, want, fresh)):
            assert np.array_equal(g.cpu().numpy(), w) and np.array_equal(fr, w), (what, i)
        assert f.view(*size) == e["view"]
        steps.append(what)

    step(big, 0, False, "first size")
    step(small, 0, False, "smaller size")
    step(big, 0, False, "first size again")
    f.configure(params_of(1, *big), True)
    step(big, 1, True, "another profile, test mode")
    f.configure(None, False)
    step(big, None, False, "no profile")
    f.configure(params_of(3, *big), False)
    step(big, 3, False, "profile 3")
    bad = (0.0,) + params_of(0, *big)[1:]
    with pytest.raises(lvk.LvkHipError):
        f.configure(bad, True)
    step(big, 3, False, "after the refused configure")
    with pytest.raises(lvk.LvkHipError):
        lvk.LCFilter((1.0, 0.0) + params_of(0, *big)[2:], context=ctx)
    assert len(steps) == 7


@pytest.mark.parametrize("layout", LAYOUTS)
def test_steady_state_allocates_nothing(ctx, lc, layout):
    """The pool has no counter to read (tests/test_scaling_420_gpu.py taps none either), so the block itself is the tap: the pool is emptied and given ONE
    block of the packed frame's size, filled with a pattern.  Every call must take that block and give it back: after the call lvk_hip_malloc of the size
    hands out the same address, and the block holds the packed frame the call made in it (the ingest with the grid) -- a call that allocated memory of
    its own would leave the pattern.  Three calls in a row."""
    size = (270, 480)
    rows, cols = size
    e = filter_expected(size, 0, True, "smooth")
    gridded = packed_expected(size, 0, True, True, "smooth")["gridded"]
    f = lc(params_of(0, *size), True)
    planes = [gpu(p) for p in layout_of(e["planes"], layout)]
    nbytes = ((3 * cols + 3) & ~3) * rows
    assert nbytes == gridded.size
    L = ctx.lib
    ctx.sync()
    assert L.lvk_hip_trim(ctx.handle) == 0
    block = ctypes.c_void_p()
    assert L.lvk_hip_malloc(ctx.handle, nbytes, ctypes.byref(block)) == 0
    pattern = np.full(nbytes, 0x5A, np.uint8)
    for _ in range(3):
        assert L.lvk_hip_upload(ctx.handle, block, pattern.ctypes.data_as(ctypes.c_void_p), nbytes) == 0
        ctx.sync()
        assert L.lvk_hip_free(ctx.handle, block) == 0
        outs = f.apply_yuv420(*planes)
        ctx.sync()
        again = ctypes.c_void_p()
        assert L.lvk_hip_malloc(ctx.handle, nbytes, ctypes.byref(again)) == 0
        assert again.value == block.value
        held = np.zeros(nbytes, np.uint8)
        assert L.lvk_hip_download(ctx.handle, held.ctypes.data_as(ctypes.c_void_p), again, nbytes) == 0
        ctx.sync()
        assert np.array_equal(held.reshape(gridded.shape), gridded)
        for o, w in zip(outs, layout_of(e["want"], layout)):
            assert np.array_equal(o.cpu().numpy(), w)
    assert L.lvk_hip_free(ctx.handle, block) == 0


@pytest.mark.parametrize("layout", LAYOUTS)
def test_refused_filter_calls_change_nothing(ctx, lc, layout):
    size = (16, 34)
    rows, cols = size
    nv12 = 1 if layout == "nv12" else 0
    e = filter_expected(size, 0, True, "random")
    planes, want = layout_of(e["planes"], layout), layout_of(e["want"], layout)
    f = lc(params_of(0, *size), True)
    ins = [Plane(p, 4, 0, seed=20 + i) for i, p in enumerate(planes)]
    outs = guarded_outputs(want, (4, 4, 4))
    n = len(planes)
    ip = [p.view.data_ptr() for p in ins] + [None] * (3 - n)
    op = [p.view.data_ptr() for p in outs] + [None] * (3 - n)
    isteps = [p.pitch for p in ins] + [0] * (3 - n)
    osteps = [p.pitch for p in outs] + [0] * (3 - n)
    before = [p.buf.cpu().numpy() for p in outs]

    def raw(i, s, o, t, sz):
        return ctx.lib.lvk_hip_lens_apply_yuv420(f.handle, i[0], s[0], i[1], s[1], i[2], s[2], o[0], t[0], o[1], t[1], o[2], t[2], sz[0], sz[1], nv12)

    def unchanged():
        ctx.sync()
        return (all(np.array_equal(p.buf.cpu().numpy(), b) for p, b in zip(outs, before)) and all(np.array_equal(p.buf.cpu().numpy(), p.flat) for p in ins))

    refused = []
    for i in range(n):                                           # a NULL plane that is in use
        refused.append((ip[:i] + [None] + ip[i + 1:], isteps, op, osteps, size))
        refused.append((ip, isteps, op[:i] + [None] + op[i + 1:], osteps, size))
    for bad in [1, 0, -2, 3, 15]:                                # odd sizes and sizes below 2
        refused.append((ip, isteps, op, osteps, (bad, cols)))
        refused.append((ip, isteps, op, osteps, (rows, bad)))
    row = [cols, cols if nv12 else cols // 2, cols // 2]
    for i in range(n):                                           # a pitch below its row
        s = list(isteps); s[i] = row[i] - 1
        refused.append((ip, s, op, osteps, size))
        s = list(osteps); s[i] = row[i] - 1
        refused.append((ip, isteps, op, s, size))
    refused.append((ip, isteps, [ip[0]] + op[1:], osteps, size))                              # in place
    refused.append((ip, isteps, [ip[n - 1] + 7] + op[1:], osteps, size))
    refused.append((ip, isteps, [op[0], ip[0] + 5] + op[2:], osteps, size))
    refused.append((ip, isteps, [op[0], op[0] + osteps[0] * (rows - 1)] + op[2:], osteps, size))
    if not nv12:
        refused.append((ip, isteps, [op[0], op[1], op[1] + 1], osteps, size))
        refused.append((ip, isteps, [op[0], op[1], ip[1]], osteps, size))
    for a in refused:
        assert raw(*a) == ERR_ARG, a
        assert unchanged(), a
    assert raw(ip[:2] + [ip[0]] if nv12 else ip, isteps, op[:2] + [ip[0]] if nv12 else op, osteps, size) == 0
    ctx.sync()
    assert_outputs(outs, want, "after the refusals")
    assert all(np.array_equal(p.buf.cpu().numpy(), p.flat) for p in ins)


# ---- the packed applies ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("test_mode", [False, True], ids=["plain", "grid"])
@pytest.mark.parametrize("fmt", [FORMAT_BGR, FORMAT_YUV], ids=["bgr", "yuv"])
@pytest.mark.parametrize("profile", [0, None], ids=profile_id)
@pytest.mark.parametrize("size", [(16, 34), (66, 258)], ids=size_id)
def test_packed_apply(ctx, lc, size, profile, fmt, test_mode):
    import torch
    e = packed_expected(size, profile, test_mode, fmt == FORMAT_YUV)
    f = lc(params_of(profile, *size), test_mode)
    src = gpu(e["src"])
    out = torch.full(e["want"].shape, 0x5A, dtype=torch.uint8, device="cuda")
    assert f.apply(src, fmt, out=out) is out
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), e["want"])
    # in test mode the source carries the grid afterwards; outside it the source is untouched
    assert np.array_equal(src.cpu().numpy(), e["gridded"])
    assert test_mode == (not np.array_equal(e["gridded"], e["src"]))
    # out of place: the source as its own destination is refused, nothing drawn
    again = gpu(e["src"])
    assert ctx.lib.lvk_hip_lens_apply(f.handle, again.data_ptr(), again.stride(0), size[0], size[1], fmt, again.data_ptr(), again.stride(0)) == ERR_ARG
    assert ctx.lib.lvk_hip_lens_apply(f.handle, again.data_ptr(), again.stride(0), size[0], size[1], FORMAT_BGRA, out.data_ptr(), out.stride(0)) == ERR_ARG
    ctx.sync()
    assert np.array_equal(again.cpu().numpy(), e["src"]) and np.array_equal(out.cpu().numpy(), e["want"])


@pytest.mark.parametrize("size", [(16, 34), (66, 258)], ids=size_id)
def test_gray_and_four_channel_applies(ctx, lc, size):
    import torch
    import livevisionkit_amd as lvk
    rows, cols = size
    params = params_of(1, rows, cols)
    packed = packed_source(rows, cols, "random")
    gray = gpu(packed[..., 0])
    c4 = gpu(np.concatenate([packed, packed_source(rows, cols, "smooth")[..., :1]], axis=2))
    dmap, view = ctx.lens_map(params, rows, cols)
    assert np.array_equal(dmap.cpu().numpy(), lens_map(1, rows, cols)[0]) and tuple(view) == lens_map(1, rows, cols)[1]
    f = lc(params, False)
    got_g, got_c = f.apply(gray), f.apply(c4, FORMAT_BGRA)
    want_g, want_c = ctx.remap_map_gray(gray, dmap, bg=0), ctx.remap_map_c4(c4, dmap, bg=(0, 0, 0, 0))
    ctx.sync()
    assert torch.equal(got_g, want_g) and torch.equal(got_c, want_c)
    # ... which the oracle defines (DESIGN.md sections 19, 21): channel 0 of the non-YUV program on (g, c, c); the colour bytes of the three-channel remap
    o = oracle()
    g = packed[..., 0]
    assert np.array_equal(got_g.cpu().numpy(), o.remap_map(np.stack([g, g, g], axis=2), lens_map(1, rows, cols)[0], bg=(0, 0, 0), yuv=False)[..., 0])
    assert np.array_equal(got_c.cpu().numpy()[..., :3], o.remap_map(packed, lens_map(1, rows, cols)[0], bg=(0, 0, 0), yuv=False))
    assert not np.array_equal(got_g.cpu().numpy(), g)
    # no profile: a copy
    f.configure(None, False)
    copy_g, copy_c = f.apply(gray), f.apply(c4, FORMAT_BGRA)
    ctx.sync()
    assert torch.equal(copy_g, gray) and torch.equal(copy_c, c4)
    # test mode: refused, the destination unchanged
    for profile in (params, None):
        f.configure(profile, True)
        for frame in (gray, c4):
            out = torch.full(tuple(frame.shape), 0x5A, dtype=torch.uint8, device="cuda")
            with pytest.raises(lvk.LvkHipError):
                f.apply(frame, FORMAT_BGRA, out=out)
            ctx.sync()
            assert bool((out == 0x5A).all())
