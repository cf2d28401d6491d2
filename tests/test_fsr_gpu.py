"""The FSR EASU scaler on the MI355X (lvk_hip_fsr_easu, livevisionkit_amd.FSRFilter), bit for bit against the numpy restatement
(tests/np_fsr.py).

Frames sit in wider device buffers at chosen byte offsets and pitches; every byte of the destination buffer outside the output frame (pitch
padding, guard bytes before and after) must come back unchanged."""
import ctypes

import numpy as np
import pytest

from tests import np_fsr as nf
from tests.test_cas_gpu import Buffer, content

pytestmark = pytest.mark.gpu

BGR, BGRA, RGB, RGBA, YUV, GRAY = 0, 1, 2, 3, 4, 5
FORMATS = [BGR, BGRA, RGB, RGBA, YUV]
STAGED, DIRECT = 0, 1


def run(ctx, src, dst, fmt, region, out_rows, out_cols, rows=None, cols=None, src_step=None, dst_step=None, src_ptr=None, dst_ptr=None):
    reg = None if region is None else (ctypes.c_int * 4)(*region)
    return ctx.lib.lvk_hip_fsr_easu(ctx.handle, src.ptr if src_ptr is None else src_ptr, src.step if src_step is None else src_step,
                                    src.rows if rows is None else rows, src.cols if cols is None else cols, fmt, reg,
                                    dst.ptr if dst_ptr is None else dst_ptr, dst.step if dst_step is None else dst_step, out_rows, out_cols)


def check(ctx, img, fmt, region, out_rows, out_cols, src_pad=0, dst_pad=0, src_off=0, dst_off=0, seed=0):
    rows, cols, ch = img.shape
    src = Buffer(rows, cols, ch, cols * ch + src_pad, src_off, seed, img)
    dst = Buffer(out_rows, out_cols, ch, out_cols * ch + dst_pad, dst_off, seed + 1)
    assert run(ctx, src, dst, fmt, region, out_rows, out_cols) == 0, ctx.lib.lvk_hip_last_error(ctx.handle)
    ctx.sync()
    want = dst.host.copy()
    dst.put(want, nf.fsr(img, fmt, region, out_rows, out_cols))
    got = dst.dev.cpu().numpy()
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    assert np.array_equal(src.dev.cpu().numpy(), src.host)           # the source is only read


SMALL_IN = [(1, 1), (1, 2), (2, 1), (3, 5), (16, 64), (17, 65)]
SMALL_OUT = [(1, 1), (1, 7), (5, 1), (2, 3), (7, 11), (16, 64), (33, 130), (65, 17)]


@pytest.mark.parametrize("rows,cols", SMALL_IN)
def test_small_inputs_at_many_output_sizes(ctx, rows, cols):
    img = content(rows, cols, 3, seed=rows * 100 + cols)
    for k, (oh, ow) in enumerate(SMALL_OUT):
        check(ctx, img, BGR, (0, 0, cols, rows), oh, ow, seed=k)


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format(ctx, fmt):
    ch = nf.CHANNELS[fmt]
    img = content(45, 77, ch, seed=fmt)
    for oh, ow in ((90, 154), (30, 50), (45, 200)):
        check(ctx, img, fmt, (0, 0, 77, 45), oh, ow, seed=fmt)


@pytest.mark.parametrize("region", [(0, 0, 20, 15), (37, 0, 20, 15), (0, 25, 20, 15), (37, 25, 20, 15), (1, 1, 55, 38), (56, 39, 1, 1),
                                    (0, 0, 57, 1)])
def test_crops_touching_each_frame_edge(ctx, region):
    img = content(40, 57, 4, seed=sum(region))
    for oh, ow in ((region[3] * 2, region[2] * 2), (31, 17), (1, 1)):
        check(ctx, img, RGBA, region, oh, ow)


@pytest.mark.parametrize("rows,cols,region,oh,ow,fmt", [
    (1080, 1920, (0, 0, 1920, 1080), 2160, 3840, BGRA),
    (1080, 1920, (0, 0, 1920, 1080), 2160, 3840, BGR),
    (2160, 3840, (0, 0, 3840, 2160), 1080, 1920, BGR),
    (720, 1280, (0, 0, 1280, 720), 2304, 4096, YUV),
    (1080, 1920, (480, 270, 960, 540), 1080, 1920, RGBA),
])
def test_frame_sizes(ctx, rows, cols, region, oh, ow, fmt):
    check(ctx, content(rows, cols, nf.CHANNELS[fmt], seed=rows + cols), fmt, region, oh, ow)


@pytest.mark.parametrize("region,oh,ow", [((0, 0, 1920, 1080), 2160, 3840), ((480, 270, 960, 540), 1080, 1920)])
def test_1080p_is_the_compiled_reference_shader(ctx, region, oh, ow):
    """lvk_hip_fsr_easu against the reference's own shader text (oracle/_ref/libffx_ref.so: fsr.effect's EASU pixel shader and
    FsrEasuCon) between the specification's load and store, with no numpy filter in between.  BGRA: the shader's r, g, b are bytes
    2, 1, 0 and its 4th component is stored as it returns it."""
    from tests import ffx_ref_lib
    from tests.np_cas import UNIT
    ref = ffx_ref_lib.load()
    rows, cols = 1080, 1920
    img = content(rows, cols, 4, seed=oh)
    src = Buffer(rows, cols, 4, cols * 4, 0, 1, img)
    dst = Buffer(oh, ow, 4, ow * 4, 0, 2)
    assert run(ctx, src, dst, BGRA, region, oh, ow) == 0, ctx.lib.lvk_hip_last_error(ctx.handle)
    ctx.sync()
    x = UNIT[img]
    y, dev = ref.easu_unit(x[..., 2], x[..., 1], x[..., 0], region, oh, ow)
    assert dev < 0.25, dev
    q = np.rint(y * np.float32(255)).astype(np.uint8)
    want = np.stack([q[..., 2], q[..., 1], q[..., 0], q[..., 3]], -1)
    got = dst.dev.cpu().numpy()[:oh * ow * 4].reshape(oh, ow, 4)
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())


@pytest.mark.parametrize("src_pad,dst_pad", [(1, 13), (13, 64), (64, 1), (0, 13)])
@pytest.mark.parametrize("src_off,dst_off", [(1, 2), (3, 0), (0, 3), (2, 1)])
@pytest.mark.parametrize("fmt", [BGR, RGBA])
def test_padded_pitches_and_unaligned_pointers(ctx, src_pad, dst_pad, src_off, dst_off, fmt):
    for rows, cols, oh, ow in ((37, 131, 50, 201), (5, 70, 3, 35), (2, 3, 4, 5)):
        img = content(rows, cols, nf.CHANNELS[fmt], seed=src_pad * 7 + dst_pad + src_off)
        check(ctx, img, fmt, (0, 0, cols, rows), oh, ow, src_pad, dst_pad, src_off, dst_off, seed=dst_off)


def test_alpha_is_written_as_255(ctx):
    img = content(33, 47, 4, seed=12)
    img[..., 3] = 0
    src = Buffer(33, 47, 4, 47 * 4, 0, 1, img)
    dst = Buffer(66, 94, 4, 94 * 4, 0, 2)
    assert run(ctx, src, dst, BGRA, (0, 0, 47, 33), 66, 94) == 0
    ctx.sync()
    got = dst.dev.cpu().numpy()[:66 * 94 * 4].reshape(66, 94, 4)
    assert (got[..., 3] == 255).all()


def test_staged_path(ctx):
    lib = ctx.lib
    for rows, cols, region, oh, ow in ((300, 500, (0, 0, 500, 300), 700, 1100), (300, 500, (3, 5, 400, 250), 250, 400),
                                       (300, 500, (0, 0, 500, 300), 1, 1)):
        assert lib.lvk_hip_fsr_easu_path(region[2], region[3], oh, ow) == STAGED
        check(ctx, content(rows, cols, 3, seed=oh), YUV, region, oh, ow)


def test_direct_path(ctx):
    lib = ctx.lib
    for rows, cols, region, oh, ow in ((300, 500, (0, 0, 500, 300), 150, 250), (300, 500, (0, 0, 500, 300), 30, 400),
                                       (300, 500, (7, 2, 480, 290), 290, 100), (300, 500, (0, 0, 500, 300), 200, 333),
                                       (300, 500, (0, 0, 500, 300), 5, 7)):
        assert lib.lvk_hip_fsr_easu_path(region[2], region[3], oh, ow) == DIRECT, (region, oh, ow)
        check(ctx, content(rows, cols, 4, seed=oh), BGRA, region, oh, ow)


def test_refused_calls_leave_the_destination_untouched(ctx):
    import torch
    rows, cols, oh, ow = 9, 13, 14, 20
    img = content(rows, cols, 4, seed=3)
    src = Buffer(rows, cols, 4, cols * 4 + 5, 1, 3, img)
    dst = Buffer(oh, ow, 4, ow * 4 + 3, 2, 4)
    whole = (0, 0, cols, rows)
    refused = [
        dict(fmt=GRAY), dict(fmt=6), dict(fmt=-1),
        dict(rows=0), dict(rows=-1), dict(cols=0), dict(cols=-3), dict(oh=0), dict(ow=0), dict(oh=-2),
        dict(region=(0, 0, 0, rows)), dict(region=(0, 0, cols, 0)), dict(region=(-1, 0, cols, rows)), dict(region=(0, -1, 4, 4)),
        dict(region=(1, 0, cols, rows)), dict(region=(0, 1, cols, rows)), dict(region=(cols, 0, 1, 1)), dict(region=None),
        dict(src_step=cols * 4 - 1), dict(dst_step=ow * 4 - 1), dict(fmt=BGR, src_step=cols * 3 - 1),
        dict(src_ptr=0), dict(dst_ptr=0),
    ]
    for kw in refused:
        fmt = kw.pop("fmt", BGRA)
        region = kw.pop("region", whole)
        o_h, o_w = kw.pop("oh", oh), kw.pop("ow", ow)
        assert run(ctx, src, dst, fmt, region, o_h, o_w, **kw) == -1, (fmt, region, kw)
    ctx.sync()
    assert np.array_equal(dst.dev.cpu().numpy(), dst.host)
    assert np.array_equal(src.dev.cpu().numpy(), src.host)
    # overlapping source and destination: in place, shifted by a byte, the destination's last row over the source's first
    span = (rows - 1) * src.step + cols * 4
    for dptr in (src.ptr, src.ptr + 1, src.ptr - 1, src.ptr - (oh - 1) * dst.step - ow * 4 + 1, src.ptr + span - 1):
        assert run(ctx, src, dst, BGRA, whole, oh, ow, dst_ptr=dptr) == -1, dptr - src.ptr
    ctx.sync()
    assert np.array_equal(src.dev.cpu().numpy(), src.host)
    # adjacent but disjoint ranges in one buffer are accepted: the destination starts one byte after the source's last byte
    both = Buffer(rows + oh, ow, 4, ow * 4, 0, 5)
    host = both.host.copy()
    for y in range(rows):
        host[y * ow * 4:y * ow * 4 + cols * 4] = img[y].reshape(-1)
    both.dev.copy_(torch.from_numpy(host))
    sspan = (rows - 1) * ow * 4 + cols * 4
    assert run(ctx, both, both, BGRA, whole, oh, ow, rows=rows, cols=cols, src_step=ow * 4, dst_ptr=both.ptr + sspan, dst_step=ow * 4) == 0
    ctx.sync()
    want = host.copy()
    for y, row in enumerate(nf.fsr(img, BGRA, whole, oh, ow)):
        want[sspan + y * ow * 4:sspan + y * ow * 4 + ow * 4] = row.reshape(-1)
    assert np.array_equal(both.dev.cpu().numpy(), want)


def test_python_filter(ctx):
    import torch
    import livevisionkit_amd as lvk
    f = lvk.FSRFilter(ctx, multiplier=2.0)
    img = content(45, 77, 3, seed=9)
    out = f.apply(torch.from_numpy(img).cuda(), YUV)
    ctx.sync()
    assert out.shape == (90, 154, 3)
    assert np.array_equal(out.cpu().numpy(), nf.fsr_filter(img, YUV, multiplier=2.0))
    # an explicit size with the aspect fit and a crop, a padded view in, a caller's buffer out
    wide = torch.from_numpy(content(45, 80, 4, seed=10)).cuda()
    view = wide[:, :77]
    f.configure(output_size=(100, 100), maintain_aspect_ratio=True, crop=(5, 3, 2, 0))
    region, (oh, ow), skip = f.geometry(45, 77)
    assert region == (5, 3, 70, 42) and (oh, ow) == (60, 100) and not skip
    dst = torch.full((oh, ow, 4), 7, dtype=torch.uint8, device="cuda")
    assert f.apply(view, RGBA, out=dst) is dst
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), nf.fsr_filter(view.cpu().numpy(), RGBA, (100, 100), 1.0, True, (5, 3, 2, 0)))
    # pass-through: same size, whole frame
    f.configure(multiplier=1.0)
    frame = torch.from_numpy(img).cuda()
    assert f.apply(frame, BGR) is frame
    # a mid-stream change of the input size: the output follows the current frame
    f.configure(multiplier=0.5)
    for rows, cols in ((40, 60), (41, 63), (40, 60)):
        im = content(rows, cols, 3, seed=rows + cols)
        got = f.apply(torch.from_numpy(im).cuda(), BGR)
        ctx.sync()
        assert np.array_equal(got.cpu().numpy(), nf.fsr_filter(im, BGR, multiplier=0.5))
    for bad in (dict(multiplier=0.0), dict(multiplier=float("nan")), dict(crop=(0, 0, 4097, 0)), dict(crop=(-1, 0, 0, 0)),
                dict(output_size=(-1, 5))):
        with pytest.raises(ValueError):
            f.configure(**bad)
    with pytest.raises(ValueError):
        f.apply(frame, GRAY)
    with pytest.raises(ValueError):
        f.apply(frame, BGR, out=torch.empty((3, 3, 3), dtype=torch.uint8, device="cuda"))
    assert f.multiplier == 0.5
