"""Format conversion on the MI355X (lvk_hip_reformat, livevisionkit_amd.reformat / ConversionFilter), bit for bit against the numpy
restatement (tests/np_convert.py).

Frames sit in wider device buffers at chosen byte offsets and pitches; every byte of the destination buffer outside the frame (pitch
padding, guard bytes before and after) must come back unchanged."""
import numpy as np
import pytest

from tests import np_convert as nc

pytestmark = pytest.mark.gpu

BGR, BGRA, RGB, RGBA, YUV, GRAY = nc.FORMATS
ALL_PAIRS = sorted(nc.PAIRS) + [(f, f) for f in nc.FORMATS]          # the 30 conversions and the 6 copies
GUARD = 64


def content(rows, cols, ch, seed):
    """Random bytes with a flat patch and a ramp."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (rows, cols, ch), dtype=np.uint8)
    if rows >= 4 and cols >= 4:
        img[: rows // 2, : cols // 2] = rng.integers(0, 256, ch, dtype=np.uint8)
        img[rows // 2:, cols // 2:, 0] = (np.arange(cols) * 255 // max(cols - 1, 1)).astype(np.uint8)[cols // 2:]
    return img


class Buffer:
    """A device buffer of random guard bytes holding a [rows, cols, ch] frame at byte `offset` with row pitch `step`."""

    def __init__(self, rows, cols, ch, step, offset, seed, img=None):
        import torch
        self.rows, self.cols, self.ch, self.step, self.offset = rows, cols, ch, step, offset
        self.host = np.random.default_rng(seed).integers(0, 256, offset + (rows - 1) * step + cols * ch + GUARD, dtype=np.uint8)
        if img is not None:
            self.put(self.host, img)
        self.dev = torch.from_numpy(self.host.copy()).cuda()

    def put(self, buf, img):
        if self.step == self.cols * self.ch:
            buf[self.offset:self.offset + img.size] = img.reshape(-1)
            return
        for y in range(self.rows):
            o = self.offset + y * self.step
            buf[o:o + self.cols * self.ch] = img[y].reshape(-1)

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.offset


def run(ctx, src, dst, sf, df, rows=None, cols=None, src_step=None, dst_step=None, src_ptr=None, dst_ptr=None):
    return ctx.lib.lvk_hip_reformat(ctx.handle, src.ptr if src_ptr is None else src_ptr, src.step if src_step is None else src_step,
                                    src.rows if rows is None else rows, src.cols if cols is None else cols, sf,
                                    dst.ptr if dst_ptr is None else dst_ptr, dst.step if dst_step is None else dst_step, df)


def check(ctx, img, sf, df, src_pad=0, dst_pad=0, src_off=0, dst_off=0, seed=0):
    rows, cols, sc = img.shape
    dc = nc.CHANNELS[df]
    src = Buffer(rows, cols, sc, cols * sc + src_pad, src_off, seed, img)
    dst = Buffer(rows, cols, dc, cols * dc + dst_pad, dst_off, seed + 1)
    assert run(ctx, src, dst, sf, df) == 0, ctx.lib.lvk_hip_last_error(ctx.handle)
    ctx.sync()
    want = dst.host.copy()
    dst.put(want, nc.reformat(img, sf, df))
    got = dst.dev.cpu().numpy()
    assert np.array_equal(got, want), "%s -> %s: %d bytes differ" % (nc.NAMES[sf], nc.NAMES[df], int((got != want).sum()))
    assert np.array_equal(src.dev.cpu().numpy(), src.host)           # the source is only read


SIZES = [(1, 1), (1, 3), (2, 5), (17, 65), (270, 480), (1080, 1920), (2160, 3840)]


@pytest.mark.parametrize("rows,cols", SIZES)
@pytest.mark.parametrize("sf,df", ALL_PAIRS)
def test_every_pair_and_copy_at_every_size(ctx, sf, df, rows, cols):
    check(ctx, content(rows, cols, nc.CHANNELS[sf], seed=rows * 7 + cols + 13 * sf + df), sf, df, seed=sf * 6 + df)


def _every_triple():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([a & 255, (a >> 8) & 255, a >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.mark.parametrize("sf,df", [(BGR, YUV), (RGB, YUV), (YUV, BGR), (YUV, RGBA)])
def test_every_input_value(ctx, sf, df):
    import torch
    from livevisionkit_amd import reformat
    img = _every_triple()
    got = reformat(ctx, torch.from_numpy(img).cuda(), sf, df)
    ctx.sync()
    assert np.array_equal(got.cpu().numpy(), nc.reformat(img, sf, df))


@pytest.mark.parametrize("sf,df", ALL_PAIRS)
def test_pitches_offsets_and_guard_bytes(ctx, sf, df):
    sc = nc.CHANNELS[sf]
    cases = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 13, 0, 0), (64, 64, 0, 0), (13, 1, 1, 2), (0, 0, 3, 1), (64, 0, 2, 3), (1, 13, 3, 3), (0, 0, 4, 4)]
    for k, (sp, dp, so, do) in enumerate(cases):
        for rows, cols in ((5, 37), (9, 64), (3, 130), (4, 100)):
            check(ctx, content(rows, cols, sc, seed=k * 31 + cols), sf, df, src_pad=sp, dst_pad=dp, src_off=so, dst_off=do, seed=k)


def test_refused_calls_leave_the_destination_untouched(ctx):
    rows, cols = 6, 20
    src = Buffer(rows, cols, 3, cols * 3, 0, 1, content(rows, cols, 3, 1))
    dst = Buffer(rows, cols, 4, cols * 4, 0, 2)
    refused = [
        dict(sf=BGR, df=6), dict(sf=-1, df=BGRA), dict(sf=BGR, df=99), dict(sf=6, df=6),
        dict(sf=BGR, df=BGRA, rows=0), dict(sf=BGR, df=BGRA, cols=0), dict(sf=BGR, df=BGRA, rows=-2),
        dict(sf=BGR, df=BGRA, src_step=cols * 3 - 1), dict(sf=BGR, df=BGRA, dst_step=cols * 4 - 1),
        dict(sf=BGR, df=BGRA, src_ptr=0), dict(sf=BGR, df=BGRA, dst_ptr=0),
    ]
    for k, r in enumerate(refused):
        sf, df = r.pop("sf"), r.pop("df")
        assert run(ctx, src, dst, sf, df, **r) == -1, (k, sf, df, r)
    # overlapping byte ranges, each inside one buffer large enough to hold both frames (were one accepted, it would still write in bounds)
    pool = Buffer(2 * rows, cols, 4, cols * 4, 0, 3, content(2 * rows, cols, 4, 3))
    overlaps = [
        dict(sf=BGRA, df=BGRA),                                                       # in place, a copy
        dict(sf=BGRA, df=RGBA),                                                       # in place, a conversion
        dict(sf=BGRA, df=BGR, dst_ptr=pool.ptr + 5),                                  # shifted by a few bytes
        dict(sf=BGRA, df=YUV, dst_ptr=pool.ptr + (rows - 1) * cols * 4 + 3),          # the destination starts inside the last source row
        dict(sf=GRAY, df=BGRA, src_ptr=pool.ptr + rows * cols * 4 - 1, src_step=cols),  # the last source byte is the first destination byte
    ]
    for k, r in enumerate(overlaps):
        sf, df = r.pop("sf"), r.pop("df")
        assert run(ctx, pool, pool, sf, df, rows=rows, **r) == -1, (k, sf, df, r)
    ctx.sync()
    assert np.array_equal(dst.dev.cpu().numpy(), dst.host)
    assert np.array_equal(src.dev.cpu().numpy(), src.host)
    assert np.array_equal(pool.dev.cpu().numpy(), pool.host)
    # adjacent, not overlapping, is accepted
    assert run(ctx, pool, pool, BGRA, RGBA, rows=rows, dst_ptr=pool.ptr + rows * cols * 4) == 0
    ctx.sync()
    got = pool.dev.cpu().numpy()[: 2 * rows * cols * 4].reshape(2 * rows, cols, 4)
    assert np.array_equal(got[rows:], nc.reformat(pool.host[: rows * cols * 4].reshape(rows, cols, 4), BGRA, RGBA))
    assert np.array_equal(got[:rows], pool.host[: rows * cols * 4].reshape(rows, cols, 4))


def test_python_reformat_and_conversion_filter(ctx):
    import torch
    from livevisionkit_amd import ConversionFilter, LvkHipError, reformat
    from livevisionkit_amd import convert as cv
    img = content(33, 71, 3, seed=5)
    t = torch.from_numpy(img).cuda()
    # a padded-row view: contiguous rows, a pitch of its own
    wide = torch.zeros((33, 80, 3), dtype=torch.uint8, device="cuda")
    view = wide[:, 3:74]
    reformat(ctx, t, BGR, YUV, out=view)
    ctx.sync()
    assert np.array_equal(view.cpu().numpy(), nc.reformat(img, BGR, YUV))
    assert not wide[:, :3].any() and not wide[:, 74:].any()
    for code, fmt, dcn in [(cv.COLOR_BGR2YUV, BGR, None), (cv.COLOR_BGR2YUV, BGRA, None), (cv.COLOR_YUV2BGR, YUV, 4), (cv.COLOR_YUV2RGB, YUV, None),
                           (cv.COLOR_RGBA2BGR, RGBA, None), (cv.COLOR_BGRA2RGB, BGRA, None), (cv.COLOR_GRAY2BGRA, GRAY, 4),
                           (cv.COLOR_RGB2GRAY, RGBA, 1), (cv.COLOR_BGR2RGB, RGB, 3)]:
        src = content(33, 71, nc.CHANNELS[fmt], seed=code + fmt)
        f = ConversionFilter(ctx, code, output_channels=dcn)
        out, to = f.apply(torch.from_numpy(src).cuda(), fmt)
        ctx.sync()
        want, want_to = nc.convert(src, fmt, code, 0 if dcn is None else dcn)
        assert to == want_to and np.array_equal(out.cpu().numpy(), want), (code, fmt, dcn)
    with pytest.raises(ValueError):
        ConversionFilter(ctx, cv.COLOR_YUV2BGR).apply(t, BGR)         # YUV2BGR does not take a BGR frame
    with pytest.raises(ValueError):
        reformat(ctx, t, BGR, BGRA, out=torch.empty((33, 71, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(LvkHipError):
        reformat(ctx, t, BGR, RGB, out=t)                             # in place is refused by the library
