"""GPU parity of the one-channel (GRAY) remap kernels -- homography, mesh, materialised map, lens-fused, WarpMesh::apply -- through the C-ABI.

Specification (tests/test_gray_spec.py): channel 0 of the oracle's non-YUV program on the three-channel frame (g, 128, 128),
background (bg, *, *).  Bar: bit-exact.  Every case counts its pixel classes -- background, nearest-neighbour border, EASU interior -- with the numpy twin's
rules (np_easu._remap_tail), so that no case passes on background alone."""
import numpy as np
import pytest

from tests import np_easu, synth

pytestmark = pytest.mark.gpu

f32 = np.float32
BG = 77
# 2 x 2 and 5 x 5: every pixel is border or background (the EASU interior needs 6 x 6); 63 x 65, 64 x 64, 257 x 129: the wave (64 lanes x 4 pixels), block
# (4 rows) and strip (256 columns) edges of the launch geometry; 253 .. 257 columns: the strip width -3 .. +1 (a misaligned row is shifted by up to 3 bytes)
SIZES = [(2, 2), (5, 5), (6, 7), (63, 65), (64, 64), (257, 129), (129, 257), (9, 253), (9, 255), (9, 256), (9, 257)]
LENS = lambda r, c: (0.8 * c, 0.8 * c, c / 2, r / 2, -0.12, 0.03, 0, 0, 0)


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _plane(rows, cols):
    rng = np.random.default_rng(rows * 1009 + cols)
    return synth.textured_frame(rows, cols, seed=rows + cols)[..., 0].copy() if min(rows, cols) >= 32 else rng.integers(0, 256, (rows, cols), dtype=np.uint8)


def _three(g):
    f = np.full(g.shape + (3,), 128, np.uint8)
    f[..., 0] = g
    return f


def _homographies(rows, cols):
    """identity, a sub-pixel shift, and a rotation about the centre pushed towards a corner: that corner's source lies outside the frame."""
    cx, cy = (cols - 1) / 2.0, (rows - 1) / 2.0
    th = 0.5; c, s = np.cos(th), np.sin(th)
    R = np.array([[c, -s, cx - c * cx + s * cy + 0.45 * cols], [s, c, cy - s * cx - c * cy + 0.3 * rows], [0, 0, 1]])
    return {"identity": np.eye(3, dtype=f32), "shift": np.array([[1, 0, 0.37], [0, 1, 0.61], [0, 0, 1]], f32), "rotation": R.astype(f32)}


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
    if not np.array_equal(got, want):
        d = np.abs(got.astype(np.int32) - want.astype(np.int32)); ys, xs = np.nonzero(d)
        raise AssertionError(f"{what}: {len(ys)} pixels differ, max |d| = {d.max()}, first at (x={xs[0]}, y={ys[0]}): gpu={got[ys[0], xs[0]]} oracle={want[ys[0], xs[0]]}")


@pytest.mark.parametrize("size", SIZES)
def test_homography_and_map_kernels_bit_exact(ctx, oracle, size):
    rows, cols = size
    g = _plane(rows, cols); g3 = _three(g); dg = _gpu(g)
    yy, xx = np.mgrid[0:rows, 0:cols]
    for kind, H in _homographies(rows, cols).items():
        subx, suby = _coords_h(H, rows, cols)
        _expect_classes(kind, _classes(subx, suby, rows, cols), rows, cols, f"homography {kind} {size}")
        want = oracle.remap_homography(g3, H, bg=(BG, 1, 2), yuv=False)[..., 0]
        got = ctx.remap_homography_gray(dg, H, bg=BG); ctx.sync()
        _same(got, want, f"homography {kind} {size}")
        # the same warp as a materialised offset map (the map kernel adds the offset to the pixel's own coordinate)
        m = np.stack([subx - xx.astype(f32), suby - yy.astype(f32)], -1).astype(f32)
        _expect_classes(kind, _classes(xx.astype(f32) + m[..., 0], yy.astype(f32) + m[..., 1], rows, cols), rows, cols, f"map {kind} {size}")
        want = oracle.remap_map(g3, m, bg=(BG, 1, 2), yuv=False)[..., 0]
        got = ctx.remap_map_gray(dg, _gpu(m), bg=BG); ctx.sync()
        _same(got, want, f"map {kind} {size}")


def _meshes(rows, cols):
    """2 x 2 (the homography route), 3 x 3 and 16 x 16; identity, a sub-pixel shift, and ("rotation") offsets that carry the top-left corner out of the frame"""
    rng = np.random.default_rng(rows * 31 + cols)
    out = []
    for (mr, mc) in [(2, 2), (3, 3), (16, 16)]:
        out.append(("identity", np.zeros((mr, mc, 2), f32)))
        sh = np.zeros((mr, mc, 2), f32); sh[..., 0] = 0.37 / cols; sh[..., 1] = 0.61 / rows
        out.append(("shift", sh))
        # (the top-left quadrant of the vertices, so that the smallest frames, which sample a large mesh sparsely, see the whole offset: at 2 x 2 pixels only an offset below -1 pixel leaves the frame -- (int)(-0.9) is column 0)
        ro = synth.random_mesh(mr, mc, rng, amp=0.04); ro[:(mr + 1) // 2, :(mc + 1) // 2] = (-0.75, -0.6); ro[-1, -1] += (0.05, 0.02)
        out.append(("rotation", ro.astype(f32)))
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
    g = _plane(rows, cols); g3 = _three(g); dg = _gpu(g)
    for kind, mesh in _meshes(rows, cols):
        what = f"mesh {mesh.shape[0]}x{mesh.shape[1]} {kind} {size}"
        _expect_classes(kind, _classes(*_coords_mesh(oracle, mesh, rows, cols), rows, cols), rows, cols, what)
        want = oracle.warpmesh_apply(g3, mesh, bg=(BG, 1, 2), yuv=False)[..., 0]
        got = ctx.warpmesh_apply_gray(dg, mesh, bg=BG); ctx.sync()
        _same(got, want, "warpmesh_apply " + what)
        # the mesh kernel itself (a 2 x 2 mesh included: lvk_hip_remap_mesh_gray does not take the homography route)
        want = oracle.remap_mesh(g3, mesh, bg=(BG, 1, 2), yuv=False)[..., 0]
        got = ctx.remap_mesh_gray(dg, mesh, bg=BG); ctx.sync()
        _same(got, want, "remap_mesh " + what)


@pytest.mark.parametrize("size", [(6, 7), (63, 65), (64, 64), (257, 129), (9, 255)])
def test_lens_fused_kernels_bit_exact(ctx, oracle, size):
    rows, cols = size
    g = _plane(rows, cols); g3 = _three(g); dg = _gpu(g)
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
        assert counts[1] > 0 and (counts[2] > 0 or min(rows, cols) < 32) and (kind != "rotation" or counts[0] > 0), (kind, size, counts)
        want = oracle.warpmesh_apply_lens(g3, mesh, params, bg=(BG, 1, 2), yuv=False)
        got = ctx.warpmesh_apply_gray(dg, mesh, bg=BG, lens=params); ctx.sync()
        _same(got, want[..., 0], f"lens mesh {mesh.shape[0]}x{mesh.shape[1]} {kind} {size}")


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_padded_and_misaligned_frames_keep_their_guard_bytes(ctx, oracle, mis):
    """step > cols on both sides, an odd pitch, and a base address 0 .. 3 bytes off a dword: the kernel shifts its 4-pixel groups by the row's misalignment,
    so the rows of one frame take all four shifts; guard bytes in front of, between and behind the rows stay what they were."""
    import torch
    rows, cols, step, lead = 37, 131, 131 + 6, 64
    g = _plane(rows, cols); g3 = _three(g)
    sbuf = torch.full((lead + rows * (cols + 3) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    src = torch.as_strided(sbuf, (rows, cols), (cols + 3, 1), lead + mis)
    src.copy_(_gpu(g))
    H = _homographies(rows, cols)["rotation"]
    mesh = _meshes(rows, cols)[5][1]
    assert mesh.shape[0] == 3
    m = np.stack(_coords_mesh(oracle, mesh, rows, cols), -1).astype(f32) - np.stack(np.mgrid[0:rows, 0:cols][::-1], -1).astype(f32)
    runs = [("homography", lambda out: ctx.remap_homography_gray(src, H, bg=BG, out=out), oracle.remap_homography(g3, H, bg=(BG, 1, 2), yuv=False)[..., 0]),
            ("mesh", lambda out: ctx.remap_mesh_gray(src, mesh, bg=BG, out=out), oracle.remap_mesh(g3, mesh, bg=(BG, 1, 2), yuv=False)[..., 0]),
            ("map", lambda out: ctx.remap_map_gray(src, _gpu(m), bg=BG, out=out), oracle.remap_map(g3, m, bg=(BG, 1, 2), yuv=False)[..., 0])]
    for name, run, want in runs:
        dbuf = torch.full((lead + rows * step + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.as_strided(dbuf, (rows, cols), (step, 1), lead + mis)
        run(out); ctx.sync()
        _same(out, want, f"padded {name} mis={mis}")
        whole = dbuf.cpu().numpy().copy()
        for y in range(rows):
            whole[lead + mis + y * step: lead + mis + y * step + cols] = 0xA5
        assert (whole == 0xA5).all(), f"{name} mis={mis}: {int((whole != 0xA5).sum())} guard bytes written"
    assert (sbuf[:lead + mis] == 0xEE).all()


def test_roi_offset_and_destination_size(ctx, oracle):
    """dst smaller than src with an ROI offset (Image.cpp:121-123), as the three-channel entry takes it"""
    g = _plane(90, 120); H = synth.random_homography(90, 120, np.random.default_rng(2))
    want = oracle.remap_homography(_three(g), H, bg=(BG, 0, 0), yuv=False, dst_size=(40, 50), offset=(7, 11))[..., 0]
    got = ctx.remap_homography_gray(_gpu(g), H, bg=BG, dst_size=(40, 50), offset=(7, 11)); ctx.sync()
    _same(got, want, "roi")


def test_refusals_leave_the_destination_untouched(ctx):
    import torch
    from livevisionkit_amd.context import LvkHipError
    g = _gpu(_plane(16, 24))
    out = torch.full((16, 24), 0x5A, dtype=torch.uint8, device="cuda")
    I = np.eye(3, dtype=f32)
    with pytest.raises(LvkHipError):
        ctx.remap_homography_gray(g, I, out=g)                                      # in place: source and destination overlap
    with pytest.raises(LvkHipError):
        ctx.remap_mesh_gray(g, np.zeros((1, 2, 2), f32), out=out)                   # below WarpMesh::MinimumSize
    Hp = I.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_float))
    rc = ctx.lib.lvk_hip_remap_homography_gray(ctx.handle, g.data_ptr(), g.stride(0), 16, 24, out.data_ptr(), 23, 16, 24, 0, 0, Hp, 0)      # pitch below the row
    assert rc == -1 and b"dst_step" in ctx.lib.lvk_hip_last_error(ctx.handle)
    ctx.sync()
    assert (out == 0x5A).all()
