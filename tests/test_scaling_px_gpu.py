"""GPU parity of ScalingFilter's two kernels on one-channel (GRAY) and four-channel (BGRA / RGBA) frames: lvk_hip_upscale_gray / _c4 and
lvk_hip_sharpen_gray / _c4 against their definitions evaluated with the oracle's THREE-channel functions
(tests/scaling_px_cases.py).  Bar: bit-exact.  Every load / store path of the kernels: ragged first and last groups, the shifted strip of a misaligned
destination, byte stores at odd pitches, guard bytes beside every row, and every refusal with the destination untouched."""
import numpy as np
import pytest

from tests import scaling_px_cases as cases

pytestmark = pytest.mark.gpu
KINDS = ["gray", "c4"]
UPSCALES = [((5, 9), (31, 17)), ((8, 8), (9, 8)), ((48, 64), (64, 49)), ((67, 131), (200, 101)), ((72, 96), (192, 144)), ((270, 480), (1280, 720))]
SHARPEN_SIZES = [(1, 1), (3, 3), (2, 9), (9, 2), (4, 5), (17, 257), (33, 1030), (67, 131), (270, 480)]
ERR_ARG = -1


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frame(kind, rows, cols):
    f = cases.frame(rows, cols)
    return np.ascontiguousarray(f[..., 0]) if kind == "gray" else f


def _want_upscale(oracle, kind, f, size):
    up3 = lambda s, sz: oracle.upscale(s, sz, yuv=False)
    return cases.upscale_gray(up3, f, size, c=77) if kind == "gray" else cases.upscale_c4(up3, f, size)


def _want_sharpen(oracle, kind, f, sharpness):
    return cases.sharpen_gray(oracle.sharpen, f, sharpness) if kind == "gray" else cases.sharpen_c4(oracle.sharpen, f, sharpness)


def _upscale(ctx, kind, *a, **k):
    return (ctx.upscale_gray if kind == "gray" else ctx.upscale_c4)(*a, **k)


def _sharpen(ctx, kind, *a, **k):
    return (ctx.sharpen_gray if kind == "gray" else ctx.sharpen_c4)(*a, **k)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        d = np.abs(got.astype(np.int32) - want.astype(np.int32)).reshape(got.shape[0], got.shape[1], -1)
        ys, xs = np.nonzero(d.max(axis=2))
        raise AssertionError(f"{what}: {len(ys)} pixels differ, max |d| = {d.max()}, first at (x={xs[0]}, y={ys[0]}): gpu={got[ys[0], xs[0]]} want={want[ys[0], xs[0]]}")


def _strided(buf, kind, rows, cols, step, offset):
    """a rows x cols frame of `kind` inside the flat byte buffer `buf`: rows `step` bytes apart, the first `offset` bytes into it"""
    import torch
    return torch.as_strided(buf, (rows, cols), (step, 1), offset) if kind == "gray" else torch.as_strided(buf, (rows, cols, 4), (step, 4, 1), offset)


def _guards_untouched(buf, fill, kind, rows, cols, step, offset, what):
    whole = buf.cpu().numpy().copy()
    row = cols * (1 if kind == "gray" else 4)
    for y in range(rows):
        whole[offset + y * step: offset + y * step + row] = fill
    assert (whole == fill).all(), f"{what}: {int((whole != fill).sum())} guard bytes written"


# ---- upscale -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("src_size,dst_size", UPSCALES)
def test_upscale_bit_exact(ctx, oracle, kind, src_size, dst_size):
    f = _frame(kind, *src_size)
    got = _upscale(ctx, kind, _gpu(f), dst_size); ctx.sync()
    _same(got, _want_upscale(oracle, kind, f, dst_size), f"upscale {kind} {src_size} -> {dst_size}")


@pytest.mark.parametrize("kind", KINDS)
def test_upscale_same_size_copies_and_a_smaller_destination_is_refused(ctx, kind):
    import torch
    from livevisionkit_amd import LvkHipError
    src = _gpu(_frame(kind, 40, 56))
    out = _upscale(ctx, kind, src, (56, 40)); ctx.sync()
    assert torch.equal(out, src)
    for size in ((55, 40), (56, 39)):                                    # Image.cpp:157
        with pytest.raises(LvkHipError):
            _upscale(ctx, kind, src, size)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_upscale_padded_and_misaligned_frames_keep_their_guard_bytes(ctx, oracle, kind, mis):
    """step > BPP * cols on both sides and a destination whose rows start 0 .. 3 pixels past a 4-pixel boundary (GRAY: a base 0 .. 3 bytes off a dword and an
    odd pitch, so the rows of one frame take all four shifts of the strip); guard bytes in front of, between and behind the rows stay what they were."""
    import torch
    bpp = 1 if kind == "gray" else 4
    (rows, cols), (dw, dh) = (37, 61), (131, 59)
    f = _frame(kind, rows, cols)
    sstep, dstep, lead = bpp * (cols + 3), (dw + 6 if kind == "gray" else 4 * (dw + 3)), 64
    sbuf = torch.full((lead + rows * sstep + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    src = _strided(sbuf, kind, rows, cols, sstep, lead + bpp * mis)
    src.copy_(_gpu(f))
    dbuf = torch.full((lead + dh * dstep + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = _strided(dbuf, kind, dh, dw, dstep, lead + bpp * mis)
    _upscale(ctx, kind, src, (dw, dh), out=out); ctx.sync()
    _same(out, _want_upscale(oracle, kind, f, (dw, dh)), f"padded upscale {kind} mis={mis}")
    _guards_untouched(dbuf, 0xA5, kind, dh, dw, dstep, lead + bpp * mis, f"upscale {kind} mis={mis}")


@pytest.mark.parametrize("kind", KINDS)
def test_upscale_refusals_leave_the_destination_untouched(ctx, kind):
    import torch
    bpp = 1 if kind == "gray" else 4
    entry = getattr(ctx.lib, "lvk_hip_upscale_" + kind)
    rows, cols, dh, dw = 12, 20, 24, 40
    src = _gpu(_frame(kind, rows, cols))
    dbuf = torch.full((8 + dh * bpp * (dw + 2) + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    out = _strided(dbuf, kind, dh, dw, bpp * (dw + 2), 8)
    args = lambda s=src, o=out, **kw: dict(dict(src=s.data_ptr(), ss=s.stride(0), sr=rows, sc=cols, dst=o.data_ptr(), ds=o.stride(0), dr=dh, dc=dw), **kw)
    call = lambda a: entry(ctx.handle, a["src"], a["ss"], a["sr"], a["sc"], a["dst"], a["ds"], a["dr"], a["dc"])
    assert call(args()) == 0                                                        # the arguments are good ones ...
    ctx.sync()
    dbuf.fill_(0x5A)
    bad = [args(src=None), args(dst=None), args(sr=0), args(sc=-1), args(dr=0), args(dc=0), args(ss=bpp * cols - 1), args(ds=bpp * dw - 1),
           args(dr=rows - 1), args(dc=cols - 1)]
    if kind == "c4":                                                                # a base or a pitch that is no multiple of 4
        sbuf = torch.zeros((rows * 4 * (cols + 1) + 8,), dtype=torch.uint8, device="cuda")
        bad += [args(s=_strided(sbuf, kind, rows, cols, 4 * cols + 4, 2)), args(s=_strided(sbuf, kind, rows, cols, 4 * cols + 2, 0)),
                args(o=_strided(dbuf, kind, dh, dw, 4 * (dw + 2), 6)), args(o=_strided(dbuf, kind, dh, dw, 4 * dw + 2, 8))]
    for a in bad:
        assert call(a) == ERR_ARG, a
    # overlap: the destination begins inside the source's byte range (and the reverse), and in place
    both = torch.full((2 * dh * bpp * dw,), 0x5A, dtype=torch.uint8, device="cuda")
    s_in = _strided(both, kind, rows, cols, bpp * cols, 0)
    for off in (0, bpp * cols * (rows - 1)):
        assert call(args(s=s_in, o=_strided(both, kind, dh, dw, bpp * dw, off))) == ERR_ARG
    s_late = _strided(both, kind, rows, cols, bpp * cols, dh * bpp * dw - 4 * bpp)
    assert call(args(s=s_late, o=_strided(both, kind, dh, dw, bpp * dw, 0))) == ERR_ARG
    ctx.sync()
    assert bool((dbuf == 0x5A).all()) and bool((both == 0x5A).all())


# ---- sharpen -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sharpness", [0.0, 0.7, 1.0])
@pytest.mark.parametrize("size", SHARPEN_SIZES)
def test_sharpen_bit_exact(ctx, oracle, kind, sharpness, size):
    f = cases.saturate_rings(_frame(kind, *size)) if size in ((67, 131), (270, 480)) else _frame(kind, *size)
    got = _sharpen(ctx, kind, _gpu(f), sharpness); ctx.sync()
    _same(got, _want_sharpen(oracle, kind, f, sharpness), f"sharpen {kind} {size} s={sharpness}")


def test_sharpen_gray_all_byte_values_and_extremes(ctx, oracle):
    """Every (ring extremum, centre) byte combination along one axis: pins the two reciprocal tables (tests/test_scaling_gpu.py's sweep on one channel)."""
    k = np.arange(256, dtype=np.uint8)
    src = np.repeat(np.repeat(k[:, None], 256, axis=1), 3, axis=0).repeat(3, axis=1)           # ring value varies with y block
    src[1::3, 1::3] = k[None, :]                                                               # centre value varies with x block
    assert src.shape == (768, 768)
    for s in (0.3, 1.0):
        got = ctx.sharpen_gray(_gpu(src), s); ctx.sync()
        _same(got, _want_sharpen(oracle, "gray", src, s), f"byte sweep s={s}")


def test_sharpen_c4_returns_a_random_alpha_byte_for_byte(ctx, oracle):
    f = cases.saturate_rings(_frame("c4", 67, 131))
    f[..., 3] = np.random.default_rng(4).integers(0, 256, f.shape[:2], dtype=np.uint8)
    got = ctx.sharpen_c4(_gpu(f), 1.0); ctx.sync()
    assert np.array_equal(got.cpu().numpy()[..., 3], f[..., 3])
    _same(got, _want_sharpen(oracle, "c4", f, 1.0), "random alpha")
    assert not np.array_equal(got.cpu().numpy()[..., :3], f[..., :3])                          # (the colours were sharpened)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("smis,dmis", [(0, 0), (1, 3), (2, 1), (3, 2), (0, 2)])
def test_sharpen_padded_and_misaligned_frames_keep_their_guard_bytes(ctx, oracle, kind, smis, dmis):
    """GRAY: source and destination bases 0 .. 3 bytes off a dword, an even pitch (dword stores in the shifted groups) and an odd one (rows that leave as
    bytes); four channels: rows that start 0 .. 3 pixels past a 16-byte boundary.  Guard bytes around every row stay what they were."""
    import torch
    bpp = 1 if kind == "gray" else 4
    rows, cols, lead = 37, 261, 64
    f = cases.saturate_rings(_frame(kind, rows, cols))
    want = _want_sharpen(oracle, kind, f, 0.6)
    for pad in (3, 6) if kind == "gray" else (3,):
        sstep, dstep = bpp * (cols + 5), bpp * (cols + pad)
        sbuf = torch.full((lead + rows * sstep + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        src = _strided(sbuf, kind, rows, cols, sstep, lead + bpp * smis)
        src.copy_(_gpu(f))
        dbuf = torch.full((lead + rows * dstep + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out = _strided(dbuf, kind, rows, cols, dstep, lead + bpp * dmis)
        _sharpen(ctx, kind, src, 0.6, out=out); ctx.sync()
        _same(out, want, f"padded sharpen {kind} mis={smis},{dmis} pitch={dstep}")
        _guards_untouched(dbuf, 0xA5, kind, rows, cols, dstep, lead + bpp * dmis, f"sharpen {kind} mis={smis},{dmis} pitch={dstep}")


@pytest.mark.parametrize("kind", KINDS)
def test_sharpen_refusals_leave_the_destination_untouched(ctx, kind):
    import torch
    bpp = 1 if kind == "gray" else 4
    entry = getattr(ctx.lib, "lvk_hip_sharpen_" + kind)
    rows, cols = 12, 20
    src = _gpu(_frame(kind, rows, cols))
    dbuf = torch.full((8 + rows * bpp * (cols + 2) + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    out = _strided(dbuf, kind, rows, cols, bpp * (cols + 2), 8)
    args = lambda s=src, o=out, **kw: dict(dict(src=s.data_ptr(), ss=s.stride(0), r=rows, c=cols, dst=o.data_ptr(), ds=o.stride(0), sharp=0.5), **kw)
    call = lambda a: entry(ctx.handle, a["src"], a["ss"], a["r"], a["c"], a["dst"], a["ds"], a["sharp"])
    assert call(args()) == 0
    ctx.sync()
    dbuf.fill_(0x5A)
    bad = [args(src=None), args(dst=None), args(r=0), args(c=-3), args(ss=bpp * cols - 1), args(ds=bpp * cols - 1),
           args(sharp=1.01), args(sharp=-0.01), args(sharp=float("nan"))]
    if kind == "c4":
        sbuf = torch.zeros((rows * 4 * (cols + 1) + 8,), dtype=torch.uint8, device="cuda")
        bad += [args(s=_strided(sbuf, kind, rows, cols, 4 * cols + 4, 2)), args(s=_strided(sbuf, kind, rows, cols, 4 * cols + 2, 0)),
                args(o=_strided(dbuf, kind, rows, cols, 4 * (cols + 2), 6)), args(o=_strided(dbuf, kind, rows, cols, 4 * cols + 2, 8))]
    for a in bad:
        assert call(a) == ERR_ARG, a
    # overlap: in place, and a destination that begins in the source's last row
    both = torch.full((2 * rows * bpp * cols,), 0x5A, dtype=torch.uint8, device="cuda")
    s_in = _strided(both, kind, rows, cols, bpp * cols, 0)
    for off in (0, bpp * cols * (rows - 1), bpp * (cols * rows - 1)):
        assert call(args(s=s_in, o=_strided(both, kind, rows, cols, bpp * cols, off))) == ERR_ARG
    ctx.sync()
    assert bool((dbuf == 0x5A).all()) and bool((both == 0x5A).all())


# ---- ScalingFilter's two steps ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_scaling_filter_chain(ctx, oracle, kind):
    """ScalingFilter::filter (ScalingFilter.cpp:52-59): upscale, then sharpen what it made"""
    f = _frame(kind, 270, 480)
    up = _upscale(ctx, kind, _gpu(f), (960, 540))
    out = _sharpen(ctx, kind, up, 0.8); ctx.sync()
    want_up = _want_upscale(oracle, kind, f, (960, 540))
    _same(up, want_up, f"chain upscale {kind}")
    _same(out, _want_sharpen(oracle, kind, want_up, 0.8), f"chain sharpen {kind}")
