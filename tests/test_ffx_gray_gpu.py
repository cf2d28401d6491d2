"""CAS and FSR EASU on one-channel frames on the MI355X (lvk_hip_cas_gray, lvk_hip_fsr_easu_gray, and CASFilter / FSRFilter of the package on
two-dimensional tensors), bit for bit against their definitions (tests/ffx_gray_cases.py evaluates them with the
three-channel specifications, and tests/test_ffx_gray_spec.py checks on the CPU that every case changes its input).

Frames sit in wider device buffers at chosen byte offsets and pitches (tests/test_cas_gpu.py's Buffer); every byte of the destination buffer
outside the frame -- pitch padding, guard bytes before and after -- must come back unchanged, and the source is only read."""
import ctypes

import numpy as np
import pytest

from tests import ffx_gray_cases as fc
from tests import np_cas as nc
from tests.test_cas_gpu import Buffer

pytestmark = pytest.mark.gpu

YUV, GRAY = 4, 5
STAGED, DIRECT = 0, 1


def run_cas(ctx, src, dst, sharpness, rows=None, cols=None, src_step=None, dst_step=None, src_ptr=None, dst_ptr=None):
    return ctx.lib.lvk_hip_cas_gray(ctx.handle, src.ptr if src_ptr is None else src_ptr, src.step if src_step is None else src_step,
                                    src.rows if rows is None else rows, src.cols if cols is None else cols,
                                    dst.ptr if dst_ptr is None else dst_ptr, dst.step if dst_step is None else dst_step, ctypes.c_float(sharpness))


def run_fsr(ctx, src, dst, region, out_rows, out_cols, rows=None, cols=None, src_step=None, dst_step=None, src_ptr=None, dst_ptr=None):
    reg = None if region is None else (ctypes.c_int * 4)(*region)
    return ctx.lib.lvk_hip_fsr_easu_gray(ctx.handle, src.ptr if src_ptr is None else src_ptr, src.step if src_step is None else src_step,
                                         src.rows if rows is None else rows, src.cols if cols is None else cols, reg,
                                         dst.ptr if dst_ptr is None else dst_ptr, dst.step if dst_step is None else dst_step, out_rows, out_cols)


def _compare(dst, src, want):
    expect = dst.host.copy()
    dst.put(expect, want)
    got = dst.dev.cpu().numpy()
    assert np.array_equal(got, expect), "%d bytes differ" % int((got != expect).sum())
    assert np.array_equal(src.dev.cpu().numpy(), src.host)           # the source is only read


def check_cas(ctx, case, sharpness, src_pad=0, dst_pad=0, src_off=0, dst_off=0, seed=0):
    img, want = fc.cas_expected(case, sharpness)
    rows, cols = img.shape
    src = Buffer(rows, cols, 1, cols + src_pad, src_off, seed, img)
    dst = Buffer(rows, cols, 1, cols + dst_pad, dst_off, seed + 1)
    assert run_cas(ctx, src, dst, sharpness) == 0, ctx.lib.lvk_hip_last_error(ctx.handle)
    ctx.sync()
    _compare(dst, src, want)


def check_fsr(ctx, case, src_pad=0, dst_pad=0, src_off=0, dst_off=0, seed=0, path=None):
    rows, cols, _, region, oh, ow, _ = case
    img, want = fc.fsr_expected(*case)
    if path is not None:
        assert ctx.lib.lvk_hip_fsr_easu_gray_path(region[2], region[3], oh, ow) == path, case
    src = Buffer(rows, cols, 1, cols + src_pad, src_off, seed, img)
    dst = Buffer(oh, ow, 1, ow + dst_pad, dst_off, seed + 1)
    assert run_fsr(ctx, src, dst, region, oh, ow) == 0, ctx.lib.lvk_hip_last_error(ctx.handle)
    ctx.sync()
    _compare(dst, src, want)


# ---------------------------------------------------------------------------------------------------------------------------------- CAS

@pytest.mark.parametrize("rows,cols", fc.CAS_SIZES)
def test_cas_sizes_at_every_sharpness(ctx, rows, cols):
    for k, s in enumerate(fc.SHARPNESS):
        check_cas(ctx, ("size", rows, cols, k), s, seed=k)


@pytest.mark.parametrize("src_pad,dst_pad", fc.PADS)
@pytest.mark.parametrize("src_off,dst_off", fc.OFFSETS)
def test_cas_padded_pitches_and_unaligned_pointers(ctx, src_pad, dst_pad, src_off, dst_off):
    for rows, cols in fc.CAS_PAD_SIZES:
        check_cas(ctx, ("pad", rows, cols), 0.8, src_pad, dst_pad, src_off, dst_off, seed=dst_off)


@pytest.mark.parametrize("dst_off", [0, 1, 2, 3])
def test_cas_every_destination_alignment_at_the_strip_width(ctx, dst_off):
    """The groups shift left by the destination's misalignment: every shift at one column below, at and above the 256-pixel strip, with a
    pitch that keeps the rows aligned alike (dword stores) and one that does not (byte stores)."""
    for cols, k in ((255, 0), (256, 1), (257, 2)):
        for dst_pad in (4 - cols % 4, 5 - cols % 4):
            check_cas(ctx, ("size", 5, cols, k), fc.SHARPNESS[k], 0, dst_pad, 0, dst_off, seed=k)


@pytest.mark.parametrize("transposed", [False, True])
def test_cas_every_byte_value_in_every_neighbour_position(ctx, transposed):
    for s in fc.CAS_SWEEP_SHARPNESS:
        check_cas(ctx, ("sweep", transposed), s)


def test_cas_flat_frames(ctx):
    for v, want_inner, want_border in ((255, 254, 254), (254, 253, 253), (128, 128, 128), (200, 200, 199)):
        check_cas(ctx, ("flat", v), 0.8)
        _, out = fc.cas_expected(("flat", v), 0.8)
        assert (out[1:-1, 1:-1] == want_inner).all() and (out[0] == want_border).all()


def test_cas_is_the_compiled_reference_shader_on_grey(ctx):
    """lvk_hip_cas_gray against the reference's own shader text (oracle/_ref/libffx_ref.so: cas.effect's pixel shader and CasSetup) on
    (g, g, g), channel 0, between the specification's load and store, with no numpy filter in between."""
    from tests import ffx_ref_lib
    ref = ffx_ref_lib.load()
    rows, cols, sharpness = fc.CAS_REF
    img = fc.cas_frame(("ref",))
    src = Buffer(rows, cols, 1, cols, 0, 1, img)
    dst = Buffer(rows, cols, 1, cols, 0, 2)
    assert run_cas(ctx, src, dst, sharpness) == 0, ctx.lib.lvk_hip_last_error(ctx.handle)
    ctx.sync()
    y = ref.cas_unit(nc.UNIT[fc.grey3(img)], ref.peak(sharpness))
    want = np.rint(y[..., 0] * np.float32(255)).astype(np.uint8)
    got = dst.dev.cpu().numpy()[:rows * cols].reshape(rows, cols)
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())


def test_cas_refused_calls_leave_the_destination_untouched(ctx):
    import torch
    rows, cols = 9, 13
    img = fc.frame(rows, cols, seed=3)
    src = Buffer(rows, cols, 1, cols + 5, 1, 3, img)
    dst = Buffer(rows, cols, 1, cols + 3, 2, 4)
    refused = [
        dict(sharpness=-0.01), dict(sharpness=1.01), dict(sharpness=float("nan")), dict(sharpness=float("inf")),
        dict(rows=0), dict(rows=-1), dict(cols=0), dict(cols=-3),
        dict(src_step=cols - 1), dict(dst_step=cols - 1), dict(src_ptr=0), dict(dst_ptr=0),
    ]
    for kw in refused:
        s = kw.pop("sharpness", 0.8)
        assert run_cas(ctx, src, dst, s, **kw) == -1, (s, kw)
    ctx.sync()
    assert np.array_equal(dst.dev.cpu().numpy(), dst.host)
    assert np.array_equal(src.dev.cpu().numpy(), src.host)
    # overlapping source and destination: in place, shifted by a byte, the destination's last row over the source's first
    for dptr in (src.ptr, src.ptr + 1, src.ptr - 1, src.ptr - (rows - 1) * src.step - cols + 1, src.ptr + (rows - 1) * src.step + cols - 1):
        assert run_cas(ctx, src, dst, 0.8, dst_ptr=dptr, dst_step=src.step) == -1, dptr - src.ptr
    ctx.sync()
    assert np.array_equal(src.dev.cpu().numpy(), src.host)
    # adjacent but disjoint ranges in one buffer are accepted: the destination starts one byte after the source's last byte
    span = (rows - 1) * src.step + cols
    both = Buffer(2 * rows, cols, 1, src.step, 0, 5)
    both.put(both.host, np.concatenate([img, np.zeros_like(img)]))
    both.dev.copy_(torch.from_numpy(both.host))
    assert run_cas(ctx, both, both, 0.8, rows=rows, dst_ptr=both.ptr + span) == 0
    ctx.sync()
    want = both.host.copy()
    for y, row in enumerate(fc.cas_gray(img, 0.8)):
        want[span + y * src.step:span + y * src.step + cols] = row
    assert np.array_equal(both.dev.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------------------- EASU

@pytest.mark.parametrize("rows,cols", fc.SMALL_IN)
def test_fsr_small_inputs_at_many_output_sizes(ctx, rows, cols):
    for k, (oh, ow) in enumerate(fc.SMALL_OUT):
        check_fsr(ctx, (rows, cols, rows * 100 + cols, (0, 0, cols, rows), oh, ow, False), seed=k)


@pytest.mark.parametrize("region", fc.CROPS)
def test_fsr_crops_touching_each_frame_edge(ctx, region):
    for oh, ow in ((region[3] * 2, region[2] * 2), (31, 17), (1, 1)):
        check_fsr(ctx, (40, 57, sum(region), region, oh, ow, True))


def test_fsr_staged_and_direct_paths(ctx):
    """The staged and direct lists of tests/test_fsr_gpu.py.  A one-channel texel is a quarter of a staged three-channel one, so some of its
    direct scales are staged here: each case runs the path lvk_hip_fsr_easu_gray_path names, and both paths run."""
    ran = set()
    for region, oh, ow in fc.STAGED_3 + fc.DIRECT_3:
        path = ctx.lib.lvk_hip_fsr_easu_gray_path(region[2], region[3], oh, ow)
        assert path in (STAGED, DIRECT)
        if (region, oh, ow) in fc.STAGED_3:
            assert path == STAGED
        check_fsr(ctx, (300, 500, oh, region, oh, ow, False), path=path)
        ran.add(path)
    assert ran == {STAGED, DIRECT}
    assert ctx.lib.lvk_hip_fsr_easu_gray_path(500, 300, 5, 7) == DIRECT and ctx.lib.lvk_hip_fsr_easu_gray_path(500, 300, 30, 400) == DIRECT


@pytest.mark.parametrize("src_pad,dst_pad", fc.PADS)
@pytest.mark.parametrize("src_off,dst_off", fc.OFFSETS)
def test_fsr_padded_pitches_and_unaligned_pointers(ctx, src_pad, dst_pad, src_off, dst_off):
    for rows, cols, oh, ow in fc.FSR_PAD_SIZES:
        check_fsr(ctx, (rows, cols, rows + cols, (0, 0, cols, rows), oh, ow, False), src_pad, dst_pad, src_off, dst_off, seed=dst_off)


@pytest.mark.parametrize("dst_off", [0, 1, 2, 3])
def test_fsr_every_destination_alignment_at_the_tile_width(ctx, dst_off):
    """Four lanes hand their bytes to the lane at the dword boundary: every alignment of the row at one column below, at and above the
    64-pixel tile, with a pitch that keeps the rows aligned alike and one that does not."""
    for oh, ow in fc.FSR_ALIGN:
        for dst_pad in (4 - ow % 4, 5 - ow % 4):
            check_fsr(ctx, (17, 65, 1765, (0, 0, 65, 17), oh, ow, False), 0, dst_pad, 0, dst_off, seed=ow)


@pytest.mark.parametrize("region,oh,ow", fc.FSR_REF)
def test_fsr_is_the_compiled_reference_shader_on_grey(ctx, region, oh, ow):
    """lvk_hip_fsr_easu_gray against the reference's own shader text (oracle/_ref/libffx_ref.so: fsr.effect's EASU pixel shader and
    FsrEasuCon) with r = g = b, channel 0, between the specification's load and store, with no numpy filter in between."""
    from tests import ffx_ref_lib
    ref = ffx_ref_lib.load()
    rows, cols = 270, 480
    img = fc.frame(rows, cols, 270)
    src = Buffer(rows, cols, 1, cols, 0, 1, img)
    dst = Buffer(oh, ow, 1, ow, 0, 2)
    assert run_fsr(ctx, src, dst, region, oh, ow) == 0, ctx.lib.lvk_hip_last_error(ctx.handle)
    ctx.sync()
    x = nc.UNIT[img]
    y, dev = ref.easu_unit(x, x, x, region, oh, ow)
    assert dev < 0.25, dev
    want = np.rint(y[..., 0] * np.float32(255)).astype(np.uint8)
    got = dst.dev.cpu().numpy()[:oh * ow].reshape(oh, ow)
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    assert np.array_equal(want, fc.fsr_expected(rows, cols, 270, region, oh, ow, False)[1])


def test_fsr_refused_calls_leave_the_destination_untouched(ctx):
    import torch
    rows, cols, oh, ow = 9, 13, 14, 20
    img = fc.frame(rows, cols, seed=3)
    src = Buffer(rows, cols, 1, cols + 5, 1, 3, img)
    dst = Buffer(oh, ow, 1, ow + 3, 2, 4)
    whole = (0, 0, cols, rows)
    refused = [
        dict(rows=0), dict(rows=-1), dict(cols=0), dict(cols=-3), dict(oh=0), dict(ow=0), dict(oh=-2),
        dict(region=(0, 0, 0, rows)), dict(region=(0, 0, cols, 0)), dict(region=(-1, 0, cols, rows)), dict(region=(0, -1, 4, 4)),
        dict(region=(1, 0, cols, rows)), dict(region=(0, 1, cols, rows)), dict(region=(cols, 0, 1, 1)), dict(region=None),
        dict(src_step=cols - 1), dict(dst_step=ow - 1), dict(src_ptr=0), dict(dst_ptr=0),
    ]
    for kw in refused:
        region = kw.pop("region", whole)
        o_h, o_w = kw.pop("oh", oh), kw.pop("ow", ow)
        assert run_fsr(ctx, src, dst, region, o_h, o_w, **kw) == -1, (region, kw)
    ctx.sync()
    assert np.array_equal(dst.dev.cpu().numpy(), dst.host)
    assert np.array_equal(src.dev.cpu().numpy(), src.host)
    # overlapping source and destination: in place, shifted by a byte, the destination's last row over the source's first
    span = (rows - 1) * src.step + cols
    for dptr in (src.ptr, src.ptr + 1, src.ptr - 1, src.ptr - (oh - 1) * dst.step - ow + 1, src.ptr + span - 1):
        assert run_fsr(ctx, src, dst, whole, oh, ow, dst_ptr=dptr) == -1, dptr - src.ptr
    ctx.sync()
    assert np.array_equal(src.dev.cpu().numpy(), src.host)
    # adjacent but disjoint ranges in one buffer are accepted: the destination starts one byte after the source's last byte
    both = Buffer(rows + oh, ow, 1, ow, 0, 5)
    host = both.host.copy()
    for y in range(rows):
        host[y * ow:y * ow + cols] = img[y]
    both.dev.copy_(torch.from_numpy(host))
    sspan = (rows - 1) * ow + cols
    assert run_fsr(ctx, both, both, whole, oh, ow, rows=rows, cols=cols, src_step=ow, dst_ptr=both.ptr + sspan, dst_step=ow) == 0
    ctx.sync()
    want = host.copy()
    for y, row in enumerate(fc.fsr_gray(img, whole, oh, ow)):
        want[sspan + y * ow:sspan + y * ow + ow] = row
    assert np.array_equal(both.dev.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------------------- both

def test_python_filters_on_two_dimensional_tensors(ctx):
    import torch
    import livevisionkit_amd as lvk
    cas, fsr = lvk.CASFilter(ctx, 0.37), lvk.FSRFilter(ctx, multiplier=2.0)
    # a padded two-dimensional view in, a padded view of a caller's buffer out
    wide = torch.from_numpy(fc.frame(45, 80, seed=10)).cuda()
    view = wide[:, :77]
    g = view.cpu().numpy()
    room = torch.full((45, 90), 7, dtype=torch.uint8, device="cuda")
    out = room[:, 3:80]
    assert cas.apply(view, out=out) is out
    ctx.sync()
    want = np.full((45, 90), 7, np.uint8)
    want[:, 3:80] = fc.cas_gray(g, 0.37)
    assert np.array_equal(room.cpu().numpy(), want)
    fresh = cas.apply(view, GRAY)
    ctx.sync()
    assert fresh.shape == (45, 77) and np.array_equal(fresh.cpu().numpy(), want[:, 3:80])
    # FSR: the multiplier, then an explicit size with the aspect fit and a crop into a caller's padded buffer
    up = fsr.apply(view)
    ctx.sync()
    assert up.shape == (90, 154) and np.array_equal(up.cpu().numpy(), fc.fsr_gray(g, (0, 0, 77, 45), 90, 154))
    fsr.configure(output_size=(100, 100), maintain_aspect_ratio=True, crop=(5, 3, 2, 0))
    region, (oh, ow), skip = fsr.geometry(45, 77)
    assert region == (5, 3, 70, 42) and (oh, ow) == (60, 100) and not skip
    room = torch.full((60, 111), 9, dtype=torch.uint8, device="cuda")
    out = room[:, 1:101]
    assert fsr.apply(view, GRAY, out=out) is out
    ctx.sync()
    want = np.full((60, 111), 9, np.uint8)
    want[:, 1:101] = fc.fsr_gray(g, region, oh, ow)
    assert np.array_equal(room.cpu().numpy(), want)
    # pass-through: same size, whole frame
    fsr.configure(multiplier=1.0)
    assert fsr.apply(view) is view
    fsr.configure(multiplier=2.0)
    # a two-dimensional tensor is a GRAY frame; `out` has its shape; in place is refused by the library
    for f in (cas, fsr):
        with pytest.raises(ValueError):
            f.apply(view, YUV)
        with pytest.raises(ValueError):
            f.apply(view, out=torch.empty((45, 77, 1), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            f.apply(wide.t())                                            # rows are not contiguous
    with pytest.raises(lvk.LvkHipError):
        cas.apply(view, out=view)
    # ... and a three-dimensional one is not, whatever `fmt` says
    with pytest.raises(ValueError):
        cas.apply(view[..., None], GRAY)
    with pytest.raises(ValueError):
        fsr.apply(view[..., None], GRAY)


def test_a_gray_frame_through_fsr_then_cas(ctx):
    import torch
    import livevisionkit_amd as lvk
    g = fc.frame(33, 47, seed=12)
    up = lvk.FSRFilter(ctx, multiplier=2.0).apply(torch.from_numpy(g).cuda())
    out = lvk.CASFilter(ctx, 0.8).apply(up)
    ctx.sync()
    scaled = fc.fsr_gray(g, (0, 0, 47, 33), 66, 94)
    want = fc.cas_gray(scaled, 0.8)
    assert out.shape == (66, 94) and np.array_equal(out.cpu().numpy(), want)
    assert (want != scaled).mean() >= fc.LIVE
