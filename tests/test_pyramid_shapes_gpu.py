"""pyrDown, the Scharr derivative image and the whole optical-flow pyramid at the sizes where their index arithmetic can go wrong: one row, one
column, widths on either side of a 64-lane block, pitched planes at odd bases, and for the fused three-level launch (k_pyr_fused3: 53 x 53 ->
25 x 25 -> 11 x 11 LDS windows, reflect-101 per level) every parity of every level's size.  Bit for bit against the oracle, through the C-ABI."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (5, 1), (1, 64), (1, 65), (7, 63), (4, 129), (9, 128)]
SRC_FILL, DST_FILL, PAD = 0xEE, 0xA5, 64


def _random(shape, salt=0):
    return np.random.default_rng([shape[0], shape[1], salt]).integers(0, 256, shape, dtype=np.uint8)


def _checker(shape):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return (((y + x) & 1) * 255).astype(np.uint8)


def _plane(img, off=0, slack=0):
    """img on the device at base offset `off` with `slack` bytes between its rows, inside a 0xEE-filled buffer: (view, buffer, host copy)."""
    import torch
    rows, cols = img.shape
    pitch = cols + slack
    host = np.full(PAD + off + rows * pitch + PAD, SRC_FILL, np.uint8)
    host[PAD + off:PAD + off + rows * pitch].reshape(rows, pitch)[:, :cols] = img
    buf = torch.from_numpy(host).cuda()
    return torch.as_strided(buf, (rows, cols), (pitch, 1), PAD + off), buf, host


@pytest.fixture(scope="module")
def small_refs(oracle):
    """The oracle's pyrDown and Scharr images of the small shapes, computed once."""
    return {shape: (_random(shape), oracle.pyr_down(_random(shape)), oracle.scharr_deriv(_random(shape))) for shape in SMALL}


@pytest.mark.parametrize("off,slack", [(0, 0), (1, 3)])
@pytest.mark.parametrize("shape", SMALL)
def test_pyr_down_small_shapes_pitched_destination(ctx, small_refs, shape, off, slack):
    import torch
    img, want, _ = small_refs[shape]
    view, sbuf, shost = _plane(img, off, slack)
    drows, dcols = want.shape
    # contiguous destination ...
    got = ctx.pyr_down(view)
    ctx.sync()
    assert np.array_equal(got.cpu().numpy(), want)
    # ... and a pitched one at an odd base inside guards
    step, doff = dcols + 5, PAD + 1 + shape[1] % 4
    dbuf = torch.full((doff + drows * step + PAD,), DST_FILL, dtype=torch.uint8, device="cuda")
    out = torch.as_strided(dbuf, (drows, dcols), (step, 1), doff)
    ctx.pyr_down(view, out=out)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), want)
    out.fill_(DST_FILL)
    assert bool((dbuf == DST_FILL).all()), "a byte outside the destination window was written"
    assert np.array_equal(sbuf.cpu().numpy(), shost)


@pytest.mark.parametrize("off,slack", [(0, 0), (1, 3)])
@pytest.mark.parametrize("shape", SMALL)
def test_scharr_small_shapes_guarded_output(ctx, small_refs, shape, off, slack):
    import torch
    img, _, want = small_refs[shape]
    view, sbuf, shost = _plane(img, off, slack)
    n = shape[0] * shape[1] * 2
    dbuf = torch.full((PAD + n + PAD,), 0x5A5A, dtype=torch.int16, device="cuda")
    out = dbuf[PAD:PAD + n].view(shape[0], shape[1], 2)
    ctx.scharr(view, out=out)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), want)
    assert bool((dbuf[:PAD] == 0x5A5A).all()) and bool((dbuf[PAD + n:] == 0x5A5A).all()), "a value outside the derivative image was written"
    assert np.array_equal(sbuf.cpu().numpy(), shost)


def _check_pyramid(ctx, oracle, img, view=None, max_level=3, win=(11, 11)):
    """Every level and every derivative image of build_pyramid against the oracle's pyrDown / Scharr chain; returns the level count."""
    import torch
    got = ctx.build_pyramid(view if view is not None else torch.from_numpy(img).cuda(), max_level=max_level, win=win)
    assert [g[0].shape for g in got] == oracle.pyramid_levels(img.shape[0], img.shape[1], max_level, win), img.shape
    cur = img
    for lvl, (g_img, g_der) in enumerate(got):
        if lvl > 0:
            cur = oracle.pyr_down(cur)
        assert np.array_equal(g_img, cur), (img.shape, lvl, int((g_img != cur).sum()))
        assert np.array_equal(g_der, oracle.scharr_deriv(cur)), (img.shape, lvl)
    return len(got)


@pytest.mark.parametrize("rows", range(89, 105))
def test_fused_pyramid_every_size_parity(ctx, oracle, rows):
    """89 is the smallest size with four levels under the 11 x 11 window; 16 consecutive sizes per axis take every parity combination at all
    three reductions (the halo arithmetic at the right and bottom edges depends on it)."""
    for cols in range(89, 105):
        assert _check_pyramid(ctx, oracle, _random((rows, cols))) == 4, (rows, cols)


@pytest.mark.parametrize("shape,levels", [((88, 104), 3), ((104, 88), 3), ((88, 88), 3), ((89, 89), 4)])
def test_level_count_boundary(ctx, oracle, shape, levels):
    """Three levels: the per-level kernels; four: the fused launch."""
    assert _check_pyramid(ctx, oracle, _random(shape, 1)) == levels


@pytest.mark.parametrize("shape", [(97, 100), (104, 89)])
def test_padded_level0(ctx, oracle, shape):
    img = _random(shape, 2)
    view, sbuf, shost = _plane(img, off=1, slack=7)
    assert _check_pyramid(ctx, oracle, img, view=view) == 4
    assert np.array_equal(sbuf.cpu().numpy(), shost)


@pytest.mark.parametrize("max_level,win", [(3, (21, 21)), (0, (11, 11)), (1, (11, 11)), (2, (11, 11))])
def test_other_windows_and_level_caps(ctx, oracle, max_level, win):
    n = _check_pyramid(ctx, oracle, _random((143, 211)), max_level=max_level, win=win)
    assert n == len(oracle.pyramid_levels(143, 211, max_level, win)) and n <= max_level + 1


@pytest.mark.parametrize("shape", [(89, 89), (96, 101), (104, 103)])
def test_saturated_and_checkerboard_content(ctx, oracle, shape):
    for img in (np.full(shape, 255, np.uint8), _checker(shape)):
        assert _check_pyramid(ctx, oracle, img) == 4
