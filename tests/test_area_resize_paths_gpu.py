"""Every kernel form of the luma + INTER_AREA downscale (lvk_launch_luma_area_resize, which the stabilizer calls on the caller's own planes)
against the CPU oracle, bit for bit, through the C-ABI: the case table of tests/area_resize_cases.py gives each row's source plane a base
offset and a pitch slack inside a 0xEE-filled buffer and the form the row must run (lvk_hip_area_resize_path); the destination is a
pitched view at an odd base inside a 0xA5-filled buffer, of which no byte outside the drows x dcols window may change."""
import numpy as np
import pytest

from tests import area_resize_cases as cases

pytestmark = pytest.mark.gpu

SRC_FILL, DST_FILL, PAD = 0xEE, 0xA5, 64


def _source(row, pixels):
    """The row's source plane on the device: (the view the kernel reads, the whole buffer, its host copy)."""
    import torch
    srows, scols = row.src
    pitch = scols * row.pix + row.slack
    host = np.full(PAD + row.off + srows * pitch + PAD, SRC_FILL, np.uint8)
    body = host[PAD + row.off:PAD + row.off + srows * pitch].reshape(srows, pitch)
    body[:, :scols * row.pix] = pixels.reshape(srows, scols * row.pix)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 4 == 0
    if row.pix == 1:
        view = torch.as_strided(buf, (srows, scols), (pitch, 1), PAD + row.off)
    else:
        view = torch.as_strided(buf, (srows, scols, row.pix), (pitch, row.pix, 1), PAD + row.off)
    return view, buf, host


def _destination(i, drows, dcols):
    import torch
    step, off = dcols + 5, PAD + i % 4
    buf = torch.full((off + drows * step + PAD,), DST_FILL, dtype=torch.uint8, device="cuda")
    return torch.as_strided(buf, (drows, dcols), (step, 1), off), buf


def _run(ctx, i, row, pixels):
    """One call: the form the library reports for the plane, the destination window, and the guard checks of both buffers."""
    view, sbuf, shost = _source(row, pixels)
    out, dbuf = _destination(i, *row.dst)
    path = ctx.area_resize_path(view, row.dst[0], row.dst[1], channel=row.ch)
    ctx.luma_area_resize(view, row.dst[0], row.dst[1], channel=row.ch, out=out)
    ctx.sync()
    got = out.cpu().numpy().copy()
    out.fill_(DST_FILL)
    assert bool((dbuf == DST_FILL).all()), "a byte outside the destination window was written"
    assert np.array_equal(sbuf.cpu().numpy(), shost), "the source buffer changed"
    return path, got


@pytest.mark.parametrize("i", range(len(cases.TABLE)), ids=cases.row_id)
def test_row_runs_its_form_and_matches_the_oracle(ctx, oracle, i):
    row = cases.TABLE[i]
    for kind in (("random", "zeros", "ones", "checker") if row.extremes else ("random",)):
        pixels = cases.content(row, kind)
        want = oracle.luma_area_resize(pixels, row.dst[0], row.dst[1], channel=row.ch)
        path, got = _run(ctx, i, row, pixels)
        assert cases.PATH_NAMES[path] == row.form, (kind, cases.PATH_NAMES[path])
        assert np.array_equal(got, want), (kind, int((got != want).sum()))


DWORD_ROWS = [i for i, r in enumerate(cases.TABLE) if r.form.startswith("FAST_DW") and r.dst == cases.DST]


@pytest.mark.parametrize("i", DWORD_ROWS, ids=cases.row_id)
def test_misaligned_twins_fall_back_and_give_the_aligned_bytes(ctx, i):
    """Each of the eight dword forms with base offsets 1, 2, 3 and pitch slacks 1, 2, 3: k_area_fast, and the bytes of the aligned run."""
    row = cases.TABLE[i]
    pixels = cases.content(row)
    path, aligned = _run(ctx, i, row, pixels)
    assert cases.PATH_NAMES[path] == row.form
    twins = [j for j, t in enumerate(cases.TABLE) if t.twin_of == i]
    assert len(twins) == 6
    for j in twins:
        path, got = _run(ctx, j, cases.TABLE[j], pixels)
        assert cases.PATH_NAMES[path] == "FAST", cases.row_id(j)
        assert np.array_equal(got, aligned), cases.row_id(j)


def test_the_table_reaches_every_form(ctx):
    """Completeness, by what the library reports (not by what the table claims): every value of the enum is reached."""
    reached = set()
    for i, row in enumerate(cases.TABLE):
        view, _, _ = _source(row, cases.content(row, "zeros"))
        reached.add(ctx.area_resize_path(view, row.dst[0], row.dst[1], channel=row.ch))
    assert reached == set(cases.PATHS.values()), sorted(set(cases.PATHS.values()) - reached)


def test_path_query_refuses_what_the_resize_refuses(ctx):
    import torch
    from livevisionkit_amd.context import LvkHipError
    plane = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    for channel in (3, -3):
        with pytest.raises(LvkHipError):
            ctx.area_resize_path(plane, 4, 4, channel=channel)
    with pytest.raises(LvkHipError):
        ctx.area_resize_path(plane[:, :, 0], 4, 4, channel=-1)          # a grey conversion needs three bytes per pixel
    lib = ctx.lib
    assert lib.lvk_hip_area_resize_path(ctx.handle, plane.data_ptr(), 23, 3, 0, 8, 8, 4, 4) < 0      # pitch shorter than the row
    assert lib.lvk_hip_area_resize_path(ctx.handle, None, 24, 3, 0, 8, 8, 4, 4) < 0
