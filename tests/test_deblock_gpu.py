"""lvk::DeblockingFilter on the MI355X, bit for bit against the numpy restatement (tests/np_deblock.py)."""
import numpy as np
import pytest

from tests import deblock_px_cases as px
from tests import np_deblock as nd

pytestmark = pytest.mark.gpu

BGR, RGB, YUV = nd.FMT_BGR, nd.FMT_RGB, nd.FMT_YUV


def blocky(rows, cols, seed, block=16):
    """A compressed-looking frame: flat block x block tiles with noise of a per-tile amplitude (0-12) and a few fully textured tiles, so
    that every keep level occurs."""
    rng = np.random.default_rng(seed)
    th, tw = (rows + block - 1) // block, (cols + block - 1) // block

    def up(a):
        return np.repeat(np.repeat(a, block, axis=0), block, axis=1)[:rows, :cols]

    base, amp = up(rng.integers(0, 256, (th, tw, 3))), up(rng.integers(0, 13, (th, tw, 1)))
    f = base + np.rint((rng.random((rows, cols, 3)) * 2 - 1) * amp).astype(np.int64)
    tex = up(rng.random((th, tw)) < 0.1)
    f = np.where(tex[..., None], rng.integers(0, 256, (rows, cols, 3)), f)
    return np.clip(f, 0, 255).astype(np.uint8)


def device_frame(img, pad=0, guard_seed=0):
    """img on the GPU as a view of a wider buffer (row pitch (cols + pad) * 3) whose extra bytes hold random guard values."""
    import torch
    rows, cols = img.shape[:2]
    buf = np.random.default_rng(guard_seed).integers(0, 256, (rows, cols + pad, 3), dtype=np.uint8)
    buf[:, :cols] = img
    t = torch.from_numpy(buf).cuda()
    return t, t[:, :cols], buf


def settings(levels, bs, k, s):
    return dict(detection_levels=levels, block_size=bs, filter_size=k, filter_scaling=s)


CASES = [
    # rows, cols, format, levels, block, k, scaling, pad
    (2160, 3840, YUV, 3, 16, 5, 4.0, 0),
    (1080, 1920, BGR, 3, 16, 5, 4.0, 0),          # region 1920 x 1072
    (1080, 1920, YUV, 4, 16, 3, 2.0, 7),
    (131, 67, RGB, 1, 2, 3, 2.0, 5),
    (67, 131, YUV, 5, 16, 5, 3.0, 3),
    (1280, 720, YUV, 5, 8, 7, 3.0, 0),
    (720, 1280, BGR, 2, 32, 9, 2.5, 16),
    (720, 1280, RGB, 3, 8, 5, 4.0, 1),
    (270, 480, YUV, 2, 16, 9, 2.5, 0),
    (200, 300, BGR, 1, 2, 7, 3.0, 2),
]


@pytest.mark.parametrize("rows,cols,fmt,levels,bs,k,s,pad", CASES)
def test_apply_and_influence_bit_exact(ctx, rows, cols, fmt, levels, bs, k, s, pad):
    import livevisionkit_amd as lvk
    img = blocky(rows, cols, seed=rows + cols + k)
    want, info = nd.deblock(img, fmt, levels, bs, k, s)
    buf_t, view, buf = device_frame(img, pad, guard_seed=k)
    f = lvk.DeblockingFilter(ctx, **settings(levels, bs, k, s))
    region = f.apply(view, fmt)
    ctx.sync()
    assert region == info["region"] == f.filter_region()
    want_buf = buf.copy(); want_buf[:, :cols] = want
    got = buf_t.cpu().numpy()
    assert np.array_equal(got, want_buf), "%d bytes differ" % int((got != want_buf).sum())
    mean, grid, keep = f.grid()
    assert np.array_equal(mean, info["mean"]) and np.array_equal(grid, info["grid"]) and np.array_equal(keep, info["keep_block"])
    # the OBS filter's test mode: apply(frame, frame, true) then draw_influence(frame)
    f.draw_influence(view, fmt)
    ctx.sync()
    want_buf[:, :cols] = nd.draw_influence(want, fmt, info)
    assert np.array_equal(buf_t.cpu().numpy(), want_buf)
    f.close()


@pytest.mark.parametrize("fmt", [BGR, YUV], ids=["bgr", "yuv"])
@pytest.mark.parametrize("case", px.CASES, ids=px.case_id)
def test_small_and_edge_cases_bit_exact(ctx, case, fmt):
    # the shapes the one- and four-channel kernels are held to (tests/deblock_px_cases.py): partial downscale cells, ex = 5, blocks smaller than a wave,
    # the run-time-k LDS median, k = 115 from global memory, the 2 x 2 rule, the area tables
    import livevisionkit_amd as lvk
    img, want, info = px.expected3(case, fmt)
    rows, cols = img.shape[:2]
    buf_t, view, buf = device_frame(img, case[6], guard_seed=case[4])
    f = lvk.DeblockingFilter(ctx, **settings(*case[2:6]))
    region = f.apply(view, fmt)
    ctx.sync()
    assert region == info["region"] == f.filter_region()
    want_buf = buf.copy(); want_buf[:, :cols] = want
    got = buf_t.cpu().numpy()
    assert np.array_equal(got, want_buf), "%d bytes differ" % int((got != want_buf).sum())     # the pitch slack's guard bytes included
    _, _, RW, RH = region
    assert np.array_equal(got[RH:], buf[RH:]) and np.array_equal(got[:, RW:], buf[:, RW:])      # below and right of the region: as they were
    assert np.array_equal(f.grid()[2], info["keep_block"])
    f.close()


def test_every_keep_level_occurs_in_the_default_case(ctx):
    import livevisionkit_amd as lvk
    img = blocky(540, 960, seed=3)
    _, info = nd.deblock(img, YUV, 5, 16, 5, 4.0)
    f = lvk.DeblockingFilter(ctx, detection_levels=5)
    _, t, _ = device_frame(img)
    f.apply(t, YUV)
    _, grid, keep = f.grid()
    assert np.array_equal(grid, info["grid"])
    assert set(np.unique(np.minimum(grid, 5))) == {0, 1, 2, 3, 4, 5}


def test_large_window_reads_global_memory(ctx):
    import livevisionkit_amd as lvk
    img = blocky(132, 260, seed=8)
    want, _ = nd.deblock(img, BGR, 3, 4, 115, 4.0)       # k > 113: the median's window does not fit the LDS tile
    f = lvk.DeblockingFilter(ctx, detection_levels=3, block_size=4, filter_size=115, filter_scaling=4.0)
    buf, t, _ = device_frame(img)
    f.apply(t, BGR)
    ctx.sync()
    assert np.array_equal(buf.cpu().numpy(), want)


def test_size_change_between_calls(ctx):
    import livevisionkit_amd as lvk
    f = lvk.DeblockingFilter(ctx)
    for i, (rows, cols, fmt) in enumerate([(1080, 1920, YUV), (67, 131, BGR), (2160, 3840, RGB), (1080, 1920, YUV)]):
        img = blocky(rows, cols, seed=40 + i)
        want, info = nd.deblock(img, fmt)
        buf, t, _ = device_frame(img)
        assert f.apply(t, fmt) == info["region"]
        ctx.sync()
        assert np.array_equal(buf.cpu().numpy(), want), (rows, cols)
    f.close()


def test_configure_between_calls_and_refused_configure(ctx):
    import livevisionkit_amd as lvk
    f = lvk.DeblockingFilter(ctx)
    img = blocky(270, 480, seed=11)
    for bad in (dict(block_size=0), dict(filter_size=1), dict(filter_size=4), dict(detection_levels=0), dict(filter_scaling=1.0),
                dict(filter_scaling=float("nan"))):
        with pytest.raises(lvk.LvkHipError):
            f.configure(**bad)
        with pytest.raises(lvk.LvkHipError):
            lvk.DeblockingFilter(ctx, **bad)
    buf, t, _ = device_frame(img)
    f.apply(t, YUV)                       # still the defaults
    ctx.sync()
    assert np.array_equal(buf.cpu().numpy(), nd.deblock(img, YUV)[0])
    f.configure(detection_levels=2, block_size=8, filter_size=3, filter_scaling=2.0)
    buf, t, _ = device_frame(img)
    f.apply(t, YUV)
    ctx.sync()
    assert np.array_equal(buf.cpu().numpy(), nd.deblock(img, YUV, 2, 8, 3, 2.0)[0])


def test_refused_calls_change_nothing(ctx):
    import torch
    import livevisionkit_amd as lvk
    f = lvk.DeblockingFilter(ctx)
    img = blocky(64, 96, seed=5)
    buf, t, _ = device_frame(img)
    with pytest.raises(lvk.LvkHipError):
        f.draw_influence(t, YUV)                                  # before the first apply
    assert f.filter_region() == (0, 0, 0, 0)
    want, info = nd.deblock(img, YUV)
    f.apply(t, YUV)
    ctx.sync()
    applied = buf.cpu().numpy()
    assert np.array_equal(applied, want)
    for fmt in (1, 3, 5):                                         # BGRA, RGBA, GRAY
        with pytest.raises(lvk.LvkHipError):
            f.apply(t, fmt)
    small = blocky(15, 200, seed=6)                               # no whole 16 x 16 block
    sbuf, st, _ = device_frame(small)
    with pytest.raises(lvk.LvkHipError):
        f.apply(st, YUV)
    with pytest.raises(lvk.LvkHipError):
        f.draw_influence(st, YUV)                                 # the region (96 x 64) does not fit
    f2 = lvk.DeblockingFilter(ctx, block_size=2, filter_scaling=8.0)
    tiny = blocky(2, 2, seed=7)
    tbuf, tt, _ = device_frame(tiny)
    with pytest.raises(lvk.LvkHipError):
        f2.apply(tt, YUV)                                         # rint(2 / 8) = 0: empty downscale
    ctx.sync()
    assert np.array_equal(sbuf.cpu().numpy(), small) and np.array_equal(tbuf.cpu().numpy(), tiny)
    assert np.array_equal(buf.cpu().numpy(), applied)
    assert f.filter_region() == info["region"] and f2.filter_region() == (0, 0, 0, 0)
    # the maps of the last successful apply are still the ones draw_influence uses
    f.draw_influence(t, YUV)
    ctx.sync()
    assert np.array_equal(buf.cpu().numpy(), nd.draw_influence(applied, YUV, info))
    f.close(); f2.close()


def test_two_filters_on_one_context_are_independent(ctx):
    import livevisionkit_amd as lvk
    a = lvk.DeblockingFilter(ctx)
    b = lvk.DeblockingFilter(ctx, detection_levels=5, block_size=8, filter_size=7, filter_scaling=3.0)
    ia, ib = blocky(1080, 1920, seed=21), blocky(360, 640, seed=22)
    wa, infa = nd.deblock(ia, BGR)
    wb, infb = nd.deblock(ib, YUV, 5, 8, 7, 3.0)
    ba, ta, _ = device_frame(ia)
    bb, tb, _ = device_frame(ib)
    a.apply(ta, BGR)
    b.apply(tb, YUV)
    ctx.sync()
    assert np.array_equal(ba.cpu().numpy(), wa) and np.array_equal(bb.cpu().numpy(), wb)
    a.draw_influence(ta, BGR)
    b.draw_influence(tb, YUV)
    ctx.sync()
    assert np.array_equal(ba.cpu().numpy(), nd.draw_influence(wa, BGR, infa))
    assert np.array_equal(bb.cpu().numpy(), nd.draw_influence(wb, YUV, infb))
    assert a.filter_region() == infa["region"] and b.filter_region() == infb["region"]
    a.close(); b.close()
