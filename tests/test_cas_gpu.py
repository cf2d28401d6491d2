"""The CAS filter on the MI355X (lvk_hip_cas, livevisionkit_amd.CASFilter), bit for bit against the numpy restatement (tests/np_cas.py).

Frames sit in wider device buffers at chosen byte offsets and pitches; every byte of the destination buffer outside the frame (pitch
padding, guard bytes before and after) must come back unchanged."""
import ctypes

import numpy as np
import pytest

from tests import np_cas as nc

pytestmark = pytest.mark.gpu

BGR, BGRA, RGB, RGBA, YUV, GRAY = 0, 1, 2, 3, 4, 5
FORMATS = [BGR, BGRA, RGB, RGBA, YUV]
SHARPNESS = [0.0, 0.25, 0.37, 0.8, 1.0]
GUARD = 64


def content(rows, cols, ch, seed):
    """Random bytes with flat patches and ramps, so that every branch of the clamps is taken."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (rows, cols, ch), dtype=np.uint8)
    if rows >= 4 and cols >= 4:
        img[: rows // 2, : cols // 2] = rng.integers(0, 256, ch, dtype=np.uint8)
        ramp = (np.arange(cols) * 255 // max(cols - 1, 1)).astype(np.uint8)
        img[rows // 2:, cols // 2:, 0] = ramp[cols // 2:]
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
        for y in range(self.rows):
            o = self.offset + y * self.step
            buf[o:o + self.cols * self.ch] = img[y].reshape(-1)

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.offset


def run(ctx, src, dst, fmt, sharpness, rows=None, cols=None, src_step=None, dst_step=None, src_ptr=None, dst_ptr=None):
    lib = ctx.lib
    return lib.lvk_hip_cas(ctx.handle, src.ptr if src_ptr is None else src_ptr, src.step if src_step is None else src_step,
                           src.rows if rows is None else rows, src.cols if cols is None else cols, fmt,
                           dst.ptr if dst_ptr is None else dst_ptr, dst.step if dst_step is None else dst_step, ctypes.c_float(sharpness))


def check(ctx, img, fmt, sharpness, src_pad=0, dst_pad=0, src_off=0, dst_off=0, seed=0):
    rows, cols, ch = img.shape
    src = Buffer(rows, cols, ch, cols * ch + src_pad, src_off, seed, img)
    dst = Buffer(rows, cols, ch, cols * ch + dst_pad, dst_off, seed + 1)
    assert run(ctx, src, dst, fmt, sharpness) == 0, ctx.lib.lvk_hip_last_error(ctx.handle)
    ctx.sync()
    want = dst.host.copy()
    dst.put(want, nc.cas(img, sharpness))
    got = dst.dev.cpu().numpy()
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    assert np.array_equal(src.dev.cpu().numpy(), src.host)           # the source is only read


SMALL = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (17, 31), (16, 64), (17, 65)]


@pytest.mark.parametrize("rows,cols", SMALL)
@pytest.mark.parametrize("fmt", FORMATS)
def test_small_sizes_every_format_and_sharpness(ctx, rows, cols, fmt):
    ch = nc.CHANNELS[fmt]
    for k, s in enumerate(SHARPNESS):
        check(ctx, content(rows, cols, ch, seed=rows * 100 + cols + k), fmt, s, seed=k)


@pytest.mark.parametrize("rows,cols,fmt,sharpness", [(270, 480, BGR, 0.8), (270, 480, RGBA, 0.37), (270, 480, YUV, 1.0),
                                                     (1080, 1920, YUV, 0.8), (1080, 1920, BGRA, 0.25),
                                                     (2160, 3840, BGR, 0.8), (2160, 3840, RGBA, 0.0)])
def test_frame_sizes(ctx, rows, cols, fmt, sharpness):
    check(ctx, content(rows, cols, nc.CHANNELS[fmt], seed=rows + cols), fmt, sharpness)


@pytest.mark.parametrize("src_pad,dst_pad", [(1, 13), (13, 64), (64, 1), (0, 13)])
@pytest.mark.parametrize("src_off,dst_off", [(1, 2), (3, 0), (0, 3), (2, 1)])
@pytest.mark.parametrize("fmt", [BGR, RGBA])
def test_padded_pitches_and_unaligned_pointers(ctx, src_pad, dst_pad, src_off, dst_off, fmt):
    for rows, cols in ((37, 131), (5, 70), (2, 3)):
        img = content(rows, cols, nc.CHANNELS[fmt], seed=src_pad * 7 + dst_pad + src_off)
        check(ctx, img, fmt, 0.8, src_pad, dst_pad, src_off, dst_off, seed=dst_off)


@pytest.mark.parametrize("fmt", [BGR, BGRA])
def test_every_byte_value_in_every_neighbour_position(ctx, fmt):
    # channel c of pixel (y, x) = (x + 7 y + 85 c) mod 256 on 258 x 258 pixels, and its transpose in the other channels: each of the nine
    # positions around an interior centre sees every byte value, against centres of every value
    ch = nc.CHANNELS[fmt]
    y, x = np.mgrid[0:258, 0:258]
    img = np.stack([(x + 7 * y + 85 * c) % 256 if c % 2 == 0 else (y + 7 * x + 85 * c) % 256 for c in range(ch)], -1).astype(np.uint8)
    for s in (0.0, 0.8, 1.0):
        check(ctx, img, fmt, s)


@pytest.mark.parametrize("fmt", FORMATS)
def test_flat_frames_on_the_device(ctx, fmt):
    ch = nc.CHANNELS[fmt]
    for v, want_inner, want_border in ((255, 254, 254), (254, 253, 253), (128, 128, 128), (200, 200, 199)):
        img = np.full((20, 70, ch), v, np.uint8)
        check(ctx, img, fmt, 0.8)
        out = nc.cas(img, 0.8)
        assert (out[1:-1, 1:-1, :3] == want_inner).all() and (out[0, :, :3] == want_border).all()


def test_1080p_is_the_compiled_reference_shader(ctx):
    """lvk_hip_cas against the reference's own shader text (oracle/_ref/libffx_ref.so: cas.effect's pixel shader and CasSetup) between the
    specification's load and store, with no numpy filter in between."""
    from tests import ffx_ref_lib
    ref = ffx_ref_lib.load()
    rows, cols, sharpness = 1080, 1920, 0.8
    img = content(rows, cols, 3, seed=1080)
    src = Buffer(rows, cols, 3, cols * 3, 0, 1, img)
    dst = Buffer(rows, cols, 3, cols * 3, 0, 2)
    assert run(ctx, src, dst, BGR, sharpness) == 0, ctx.lib.lvk_hip_last_error(ctx.handle)
    ctx.sync()
    y = ref.cas_unit(nc.UNIT[img], ref.peak(sharpness))
    want = np.rint(y[..., :3] * np.float32(255)).astype(np.uint8)
    got = dst.dev.cpu().numpy()[:rows * cols * 3].reshape(rows, cols, 3)
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())


def test_refused_calls_leave_the_destination_untouched(ctx):
    import torch
    rows, cols = 9, 13
    img = content(rows, cols, 4, seed=3)
    src = Buffer(rows, cols, 4, cols * 4 + 5, 1, 3, img)
    dst = Buffer(rows, cols, 4, cols * 4 + 3, 2, 4)
    refused = [
        dict(fmt=GRAY), dict(fmt=6), dict(fmt=-1),
        dict(sharpness=-0.01), dict(sharpness=1.01), dict(sharpness=float("nan")), dict(sharpness=float("inf")),
        dict(rows=0), dict(rows=-1), dict(cols=0), dict(cols=-3),
        dict(src_step=cols * 4 - 1), dict(dst_step=cols * 4 - 1), dict(fmt=BGR, src_step=cols * 3 - 1),
        dict(src_ptr=0), dict(dst_ptr=0),
    ]
    for kw in refused:
        fmt = kw.pop("fmt", BGRA)
        s = kw.pop("sharpness", 0.8)
        assert run(ctx, src, dst, fmt, s, **kw) == -1, (fmt, s, kw)
    ctx.sync()
    assert np.array_equal(dst.dev.cpu().numpy(), dst.host)
    assert np.array_equal(src.dev.cpu().numpy(), src.host)
    # overlapping source and destination: in place, shifted by a byte, the destination's last row over the source's first
    for dptr in (src.ptr, src.ptr + 1, src.ptr - 1, src.ptr - (rows - 1) * src.step - cols * 4 + 1, src.ptr + (rows - 1) * src.step + cols * 4 - 1):
        assert run(ctx, src, dst, BGRA, 0.8, dst_ptr=dptr, dst_step=src.step) == -1, dptr - src.ptr
    ctx.sync()
    assert np.array_equal(src.dev.cpu().numpy(), src.host)
    # adjacent but disjoint ranges in one buffer are accepted: the destination starts one byte after the source's last byte
    span = (rows - 1) * src.step + cols * 4
    both = Buffer(2 * rows, cols, 4, src.step, 0, 5)
    both.put(both.host, np.concatenate([img, np.zeros_like(img)]))
    both.dev.copy_(torch.from_numpy(both.host))
    assert run(ctx, both, both, BGRA, 0.8, rows=rows, dst_ptr=both.ptr + span) == 0
    ctx.sync()
    want = both.host.copy()
    for y, row in enumerate(nc.cas(img, 0.8)):
        want[span + y * src.step:span + y * src.step + cols * 4] = row.reshape(-1)
    assert np.array_equal(both.dev.cpu().numpy(), want)


def test_python_filter(ctx):
    import torch
    import livevisionkit_amd as lvk
    f = lvk.CASFilter(ctx)
    assert f.sharpness == pytest.approx(0.8)
    img = content(45, 77, 3, seed=9)
    out = f.apply(torch.from_numpy(img).cuda(), YUV)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), nc.cas(img, 0.8))
    # a padded view in, a caller's buffer out
    wide = torch.from_numpy(content(45, 80, 4, seed=10)).cuda()
    view = wide[:, :77]
    dst = torch.full((45, 77, 4), 7, dtype=torch.uint8, device="cuda")
    f.configure(0.37)
    assert f.apply(view, RGBA, out=dst) is dst
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), nc.cas(view.cpu().numpy(), 0.37))
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            f.configure(bad)
    with pytest.raises(ValueError):
        f.apply(view, GRAY)
    with pytest.raises(lvk.LvkHipError):
        f.apply(view, RGBA, out=view)                                   # in place: refused by the library
    assert f.sharpness == pytest.approx(0.37)
