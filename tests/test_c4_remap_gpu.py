"""GPU parity of the four-channel (BGRA / RGBA) remap kernels -- homography, mesh, materialised map, lens-fused, WarpMesh::apply -- through the C-ABI.

Specification (tests/test_c4_spec.py): bytes 0 .. 2 are the oracle's non-YUV program on (c0, c1, c2) with background (b0, b1, b2),
byte 3 is channel 1 of the oracle's non-YUV program on (c0, a, a) with background (b0, b3, b3): two oracle calls per case.  Bar: bit-exact, every pixel, all
four bytes.  Every case counts its pixel classes -- background, nearest-neighbour border, EASU interior -- with the numpy twin's rules
(np_easu._remap_tail), so that no case passes on background alone.  The file also holds the tracker's view of a four-channel frame: the luma downscale at
pixel stride 4 equals the one of the three-channel frame."""
import ctypes

import numpy as np
import pytest

from tests import np_easu, synth

pytestmark = pytest.mark.gpu

f32 = np.float32
BG = (77, 201, 5, 130)                   # four distinct bytes
# 2 x 2 and 5 x 5: every pixel is border or background (the EASU interior needs 6 x 6); 63 x 65, 64 x 64, 257 x 129, 129 x 257: the wave (64 lanes x 4
# pixels), block (4 rows) and strip (256 columns) edges of the launch geometry; 253 .. 257 columns straddle the strip (a row is shifted by up to 3 pixels)
SIZES = [(2, 2), (5, 5), (6, 7), (63, 65), (64, 64), (257, 129), (129, 257), (9, 253), (9, 255), (9, 256), (9, 257)]
LENS = lambda r, c: (0.8 * c, 0.8 * c, c / 2, r / 2, -0.12, 0.03, 0, 0, 0)


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_frames = {}


def _frame(rows, cols):
    """random colour (textured where the frame is large enough to have an interior worth the name) and an alpha plane that is neither constant nor a colour plane"""
    if (rows, cols) not in _frames:
        rng = np.random.default_rng(rows * 1009 + cols)
        f = rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
        if min(rows, cols) >= 32:
            f[..., :3] = synth.textured_frame(rows, cols, seed=rows + cols)
            f[..., 3] = synth.textured_frame(rows, cols, seed=rows + cols + 7)[..., 2][::-1, ::-1]
        assert all(f[..., 3].min() != f[..., 3].max() and not np.array_equal(f[..., 3], f[..., k]) for k in range(3)) or f.size <= 16
        f.setflags(write=False)
        _frames[(rows, cols)] = f
    return _frames[(rows, cols)]


def _want(f, run):
    """the definition: run(three-channel frame, background) is one of the oracle's entries with yuv = False"""
    colour = run(np.ascontiguousarray(f[..., :3]), BG[:3])
    caa = np.ascontiguousarray(np.stack([f[..., 0], f[..., 3], f[..., 3]], -1))
    alpha = run(caa, (BG[0], BG[3], BG[3]))
    return np.concatenate([colour, alpha[..., 1:2]], -1)


def _homographies(rows, cols):
    """identity, a sub-pixel shift, and ("corner") a rotation about the centre pushed towards a corner: that corner's source lies outside the frame"""
    cx, cy = (cols - 1) / 2.0, (rows - 1) / 2.0
    th = 0.5; c, s = np.cos(th), np.sin(th)
    R = np.array([[c, -s, cx - c * cx + s * cy + 0.45 * cols], [s, c, cy - s * cx - c * cy + 0.3 * rows], [0, 0, 1]])
    return {"identity": np.eye(3, dtype=f32), "shift": np.array([[1, 0, 0.37], [0, 1, 0.61], [0, 0, 1]], f32), "corner": R.astype(f32)}


def _coords_h(H, rows, cols):
    H = np.asarray(H, f32).reshape(9)
    yy, xx = np.mgrid[0:rows, 0:cols]
    fx = xx.astype(f32); fy = yy.astype(f32)
    dz = f32(1) / (np_easu._fma(H[6], fx, H[7] * fy) + H[8])
    return fx + ((np_easu._fma(H[0], fx, H[1] * fy) + H[2]) * dz - fx), fy + ((np_easu._fma(H[3], fx, H[4] * fy) + H[5]) * dz - fy)


def _classes(subx, suby, rows, cols):
    """(background, nearest-neighbour, EASU) pixel counts by the rules of np_easu._remap_tail"""
    sx = np.trunc(np.clip(subx, -2e9, 2e9)).astype(np.int64); sy = np.trunc(np.clip(suby, -2e9, 2e9)).astype(np.int64)
    border = (sx < 1) | (sy < 1) | (sx >= cols - 4) | (sy >= rows - 4)
    inside = (sx >= 0) & (sx < cols) & (sy >= 0) & (sy < rows)
    return int((border & ~inside).sum()), int((border & inside).sum()), int((~border).sum())


def _expect_classes(kind, counts, rows, cols, what):
    """What a case must exercise.  The EASU interior exists from 6 x 6 on (1 <= sx <= cols - 5); identity and the sub-pixel shift reach it whenever it
    exists and never leave the frame; the corner warp must produce background AND border pixels at every size, and interior ones once the interior is most
    of the frame (at 6 x 7 it is two source pixels, which a rotated grid may miss)."""
    bg, nn, ea = counts
    assert nn > 0, (what, counts)
    if kind in ("identity", "shift"):
        assert bg == 0 and (ea > 0) == (rows >= 6 and cols >= 6), (what, counts)
    else:
        assert bg > 0, (what, counts)
        if min(rows, cols) >= 32:
            assert ea > 0, (what, counts)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        d = np.abs(got.astype(np.int32) - want.astype(np.int32)); ys, xs, ks = np.nonzero(d)
        raise AssertionError(f"{what}: {len(ys)} bytes differ, max |d| = {d.max()}, first at (x={xs[0]}, y={ys[0]}, byte {ks[0]}): gpu={got[ys[0], xs[0]]} oracle={want[ys[0], xs[0]]}")


@pytest.mark.parametrize("size", SIZES)
def test_homography_and_map_kernels_bit_exact(ctx, oracle, size):
    rows, cols = size
    f = _frame(rows, cols); df = _gpu(f)
    yy, xx = np.mgrid[0:rows, 0:cols]
    for kind, H in _homographies(rows, cols).items():
        subx, suby = _coords_h(H, rows, cols)
        _expect_classes(kind, _classes(subx, suby, rows, cols), rows, cols, f"homography {kind} {size}")
        want = _want(f, lambda t, bg: oracle.remap_homography(t, H, bg=bg, yuv=False))
        got = ctx.remap_homography_c4(df, H, bg=BG); ctx.sync()
        _same(got, want, f"homography {kind} {size}")
        # the same warp as a materialised offset map (the map kernel adds the offset to the pixel's own coordinate)
        m = np.stack([subx - xx.astype(f32), suby - yy.astype(f32)], -1).astype(f32)
        _expect_classes(kind, _classes(xx.astype(f32) + m[..., 0], yy.astype(f32) + m[..., 1], rows, cols), rows, cols, f"map {kind} {size}")
        want = _want(f, lambda t, bg: oracle.remap_map(t, m, bg=bg, yuv=False))
        got = ctx.remap_map_c4(df, _gpu(m), bg=BG); ctx.sync()
        _same(got, want, f"map {kind} {size}")


def _meshes(rows, cols):
    """2 x 2 (the homography route), 3 x 3, 16 x 16 and 33 x 33 (2 178 values: more than the 2 048 the kernel stages in LDS, so the global-memory arm);
    identity, a sub-pixel shift, and ("corner") offsets that carry the top-left corner out of the frame"""
    rng = np.random.default_rng(rows * 31 + cols)
    out = []
    for (mr, mc) in [(2, 2), (3, 3), (16, 16), (33, 33)]:
        out.append(("identity", np.zeros((mr, mc, 2), f32)))
        sh = np.zeros((mr, mc, 2), f32); sh[..., 0] = 0.37 / cols; sh[..., 1] = 0.61 / rows
        out.append(("shift", sh))
        # (the top-left quadrant of the vertices, so that the smallest frames, which sample a large mesh sparsely, see the whole offset: at 2 x 2 pixels only
        #  an offset below -1 pixel leaves the frame -- (int)(-0.9) is column 0)
        ro = synth.random_mesh(mr, mc, rng, amp=0.04); ro[:(mr + 1) // 2, :(mc + 1) // 2] = (-0.75, -0.6); ro[-1, -1] += (0.05, 0.02)
        out.append(("corner", ro.astype(f32)))
    return out


def _coords_mesh(oracle, mesh, rows, cols):
    yy, xx = np.mgrid[0:rows, 0:cols]
    if mesh.shape[:2] == (2, 2):
        return _coords_h(oracle.mesh2x2_to_homography(mesh, rows, cols), rows, cols)
    m = oracle.mesh_to_map(mesh, rows, cols)
    return xx.astype(f32) + m[..., 0], yy.astype(f32) + m[..., 1]


@pytest.mark.parametrize("size", SIZES)
def test_mesh_kernels_and_warpmesh_apply_bit_exact(ctx, oracle, size):
    rows, cols = size
    f = _frame(rows, cols); df = _gpu(f)
    for kind, mesh in _meshes(rows, cols):
        what = f"mesh {mesh.shape[0]}x{mesh.shape[1]} {kind} {size}"
        _expect_classes(kind, _classes(*_coords_mesh(oracle, mesh, rows, cols), rows, cols), rows, cols, what)
        want = _want(f, lambda t, bg: oracle.warpmesh_apply(t, mesh, bg=bg, yuv=False))
        got = ctx.warpmesh_apply_c4(df, mesh, bg=BG); ctx.sync()
        _same(got, want, "warpmesh_apply " + what)
        # the mesh kernel itself (a 2 x 2 mesh included: lvk_hip_remap_mesh_c4 does not take the homography route)
        want = _want(f, lambda t, bg: oracle.remap_mesh(t, mesh, bg=bg, yuv=False))
        got = ctx.remap_mesh_c4(df, mesh, bg=BG); ctx.sync()
        _same(got, want, "remap_mesh " + what)


@pytest.mark.parametrize("size", [(6, 7), (63, 65), (64, 64), (257, 129), (9, 255)])
def test_lens_fused_kernels_bit_exact(ctx, oracle, size):
    rows, cols = size
    f = _frame(rows, cols); df = _gpu(f)
    params = LENS(rows, cols)
    # the lens-fused coordinate: the warp's position in the corrected frame (background when it lies outside it), carried on by the lens map -- the numpy
    # twin reads the map where the warp points (the kernel evaluates it in closed form: a count, not a pixel comparison)
    lmap = oracle.lens_offset_map(params, rows, cols)[0]
    for kind, mesh in _meshes(rows, cols):
        u, v = _coords_mesh(oracle, mesh, rows, cols)
        ui = np.trunc(np.clip(u, -2e9, 2e9)).astype(np.int64); vi = np.trunc(np.clip(v, -2e9, 2e9)).astype(np.int64)
        ok = (ui >= 0) & (ui < cols) & (vi >= 0) & (vi < rows)
        uc, vc = np.clip(ui, 0, cols - 1), np.clip(vi, 0, rows - 1)
        counts = _classes(np.where(ok, u + lmap[vc, uc, 0], f32(-16)), np.where(ok, v + lmap[vc, uc, 1], f32(-16)), rows, cols)
        assert counts[1] > 0 and (counts[2] > 0 or min(rows, cols) < 32) and (kind != "corner" or counts[0] > 0), (kind, size, counts)
        want = _want(f, lambda t, bg: oracle.warpmesh_apply_lens(t, mesh, params, bg=bg, yuv=False))
        got = ctx.warpmesh_apply_lens_c4(df, mesh, params, bg=BG); ctx.sync()
        _same(got, want, f"lens mesh {mesh.shape[0]}x{mesh.shape[1]} {kind} {size}")


@pytest.mark.parametrize("extra", [0, 4, 8, 12])
def test_pitched_frames_keep_their_guard_bytes(ctx, oracle, extra):
    """Pitches 4 cols + 0 / 4 / 8 / 12 on both frames, with a base `extra` bytes past a 256-byte boundary: the rows of one frame start on every multiple
    of 4 modulo 16 (131 pixels a row: 524 = 12 mod 16), so the 16-byte groups take all four shifts.  Guard bytes in front of, between and behind the
    destination rows stay what they were."""
    import torch
    rows, cols, lead = 37, 131, 256
    step = 4 * cols + extra
    f = _frame(rows, cols)
    sbuf = torch.full((lead + extra + rows * step + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    src = torch.as_strided(sbuf, (rows, cols, 4), (step, 4, 1), lead + extra)
    src.copy_(_gpu(f))
    assert src.data_ptr() % 4 == 0 and len({(src.data_ptr() + y * step) % 16 for y in range(rows)}) == (1 if step % 16 == 0 else 4 if step % 8 else 2)
    H = _homographies(rows, cols)["corner"]
    mesh = _meshes(rows, cols)[5][1]
    assert mesh.shape[0] == 3
    m = np.stack(_coords_mesh(oracle, mesh, rows, cols), -1).astype(f32) - np.stack(np.mgrid[0:rows, 0:cols][::-1], -1).astype(f32)
    runs = [("homography", lambda out: ctx.remap_homography_c4(src, H, bg=BG, out=out), _want(f, lambda t, bg: oracle.remap_homography(t, H, bg=bg, yuv=False))),
            ("mesh", lambda out: ctx.remap_mesh_c4(src, mesh, bg=BG, out=out), _want(f, lambda t, bg: oracle.remap_mesh(t, mesh, bg=bg, yuv=False))),
            ("map", lambda out: ctx.remap_map_c4(src, _gpu(m), bg=BG, out=out), _want(f, lambda t, bg: oracle.remap_map(t, m, bg=bg, yuv=False)))]
    for name, run, want in runs:
        dbuf = torch.full((lead + extra + rows * step + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.as_strided(dbuf, (rows, cols, 4), (step, 4, 1), lead + extra)
        run(out); ctx.sync()
        _same(out, want, f"pitched {name} extra={extra}")
        whole = dbuf.cpu().numpy().copy()
        for y in range(rows):
            whole[lead + extra + y * step: lead + extra + y * step + 4 * cols] = 0xA5
        assert (whole == 0xA5).all(), f"{name} extra={extra}: {int((whole != 0xA5).sum())} guard bytes written"
    assert (sbuf[:lead + extra] == 0xEE).all()


def test_roi_offset_and_destination_size(ctx, oracle):
    """dst smaller than src with an ROI offset (Image.cpp:121-123), as the three-channel entry takes it"""
    f = _frame(90, 120); H = synth.random_homography(90, 120, np.random.default_rng(2))
    want = _want(f, lambda t, bg: oracle.remap_homography(t, H, bg=bg, yuv=False, dst_size=(40, 50), offset=(7, 11)))
    got = ctx.remap_homography_c4(_gpu(f), H, bg=BG, dst_size=(40, 50), offset=(7, 11)); ctx.sync()
    _same(got, want, "roi")


def test_refusals_leave_the_destination_untouched(ctx):
    import torch
    from livevisionkit_amd.context import LvkHipError
    rows, cols = 16, 24
    g = _gpu(_frame(rows, cols))
    obuf = torch.full((rows * cols * 4 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    out = obuf[:rows * cols * 4].view(rows, cols, 4)
    I = np.eye(3, dtype=f32)
    Hp = I.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    bg = (ctypes.c_uint8 * 4)(*BG)
    mesh = np.zeros((3, 3, 2), f32); mp = mesh.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    dmap = torch.zeros((rows, cols, 2), dtype=torch.float32, device="cuda")
    lens = (ctypes.c_double * 9)(*LENS(rows, cols))
    lib, h = ctx.lib, ctx.handle

    def calls(sp, ss, dp, ds):
        return [("homography", lambda: lib.lvk_hip_remap_homography_c4(h, sp, ss, rows, cols, dp, ds, rows, cols, 0, 0, Hp, bg)),
                ("mesh", lambda: lib.lvk_hip_remap_mesh_c4(h, sp, ss, rows, cols, dp, ds, mp, 3, 3, bg)),
                ("map", lambda: lib.lvk_hip_remap_map_c4(h, sp, ss, rows, cols, dp, ds, dmap.data_ptr(), dmap.stride(0) * 4, bg)),
                ("warpmesh_apply", lambda: lib.lvk_hip_warpmesh_apply_c4(h, sp, ss, rows, cols, dp, ds, mp, 3, 3, bg)),
                ("warpmesh_apply_lens", lambda: lib.lvk_hip_warpmesh_apply_lens_c4(h, sp, ss, rows, cols, dp, ds, mp, 3, 3, bg, lens))]

    S, D, step = g.data_ptr(), out.data_ptr(), 4 * cols
    bad = {"source base not a multiple of 4": (S + 2, step, D, step), "destination base not a multiple of 4": (S, step, D + 1, step),
           "source pitch not a multiple of 4": (S, step + 2, D, step), "destination pitch not a multiple of 4": (S, step, D, step + 2),
           "source step below 4 cols": (S, step - 4, D, step), "destination step below 4 cols": (S, step, D, step - 4),
           "in place": (S, step, S, step), "overlapping ranges": (S, step, S + step * (rows - 1), step),
           "null source": (None, step, D, step), "null destination": (S, step, None, step)}
    before = g.clone()
    for why, args in bad.items():
        for name, call in calls(*args):
            assert call() == -1, (why, name)                                        # LVK_HIP_ERR_ARG
    with pytest.raises(LvkHipError):
        ctx.remap_mesh_c4(g, np.zeros((1, 2, 2), f32), out=out)                   # below WarpMesh::MinimumSize
    ctx.sync()
    assert (obuf == 0x5A).all() and torch.equal(g, before)
    for name, call in calls(S, step, D, step):                                      # ... and the well-formed call goes through
        assert call() == 0, name
    ctx.sync()


# ---- the tracker's view of a four-channel frame ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [((1080, 1920), (270, 480)), ((2160, 3840), (270, 480)), ((300, 500), (127, 211)), ((120, 200), (270, 480))])
def test_luma_downscale_at_pixel_stride_4_reads_the_colour_bytes(ctx, src, dst):
    """lvk_hip_luma_area_resize at pixel stride 4 with channel -1 (BGRA) and -2 (RGBA) equals the same call on the three-channel frame: factor 4, factor 8,
    a non-integer factor and an enlarging case.  Alpha is random, so a kernel that read it would show."""
    rows, cols = src
    rng = np.random.default_rng(rows)
    bgr = synth.textured_frame(rows, cols, seed=3)
    f = np.concatenate([bgr, rng.integers(0, 256, (rows, cols, 1), dtype=np.uint8)], -1)
    d3, d4 = _gpu(bgr), _gpu(f)
    for channel in (-1, -2):
        want = ctx.luma_area_resize(d3, dst[0], dst[1], channel=channel)
        got = ctx.luma_area_resize(d4, dst[0], dst[1], channel=channel)
        ctx.sync()
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()), (src, dst, channel)
