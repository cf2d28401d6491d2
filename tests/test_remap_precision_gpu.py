"""LVK_REMAP_1LSB on the GPU, kernel by kernel, through the C-ABI against the oracle's EXACT output.

Per case, with the context in 1LSB mode: every byte within 1 of the oracle's, at most 1e-4 of a case set's bytes different at all (the two bounds that define the
mode, tests/test_remap_precision_spec.py), and every byte that never reaches the tap weights -- the border band's nearest copies and the background -- equal.
Then the context goes back to EXACT and the same call is byte-identical to the oracle again.

Which pixels reach the weights is decided here from the source coordinate in numpy (the rules of np_easu._remap_tail).  The kernel forms that coordinate with the
device reciprocal, the fused lens kernels in closed form: a pixel whose coordinate lies within EPS of a whole number may fall on either side and is held to the
"within 1" bound only; every case must still have pixels that are surely border or background, and pixels that are surely interior."""
import ctypes

import numpy as np
import pytest

from tests import np_easu_1lsb, oracle_lib, synth

pytestmark = pytest.mark.gpu

f32 = np.float32
MAX_SHARE = 1e-4
SIZES = [(67, 131), (270, 480)]            # a ragged last strip and block; both the 1-pixel and the 4-pixel border band
SIZES_EVEN = [(66, 132), (270, 480)]       # the 4:2:0 and 4:2:2 sinks need even sizes
BG = (16, 99, 201)
LENS = lambda r, c: (0.8 * c, 0.8 * c, c / 2, r / 2, -0.12, 0.03, 0, 0, 0)


@pytest.fixture(scope="module")
def pctx():
    """A context of this module's own: the precision setting must not leak into the session's shared one."""
    import livevisionkit_amd as lvk
    c = lvk.Context(0)
    yield c
    c.close()


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _texture(kind, rows, cols):
    rng = np.random.default_rng(rows * 7 + cols + len(kind))
    if kind == "noise":
        return rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    ch = np.arange(3)[None, None, :]
    s = 127.5 + 100.0 * np.sin(xx[..., None] * (0.11 + 0.03 * ch) + yy[..., None] * (0.07 - 0.02 * ch) + ch)
    return np.clip(np.round(s + rng.normal(0.0, 6.0, (rows, cols, 3))), 0, 255).astype(np.uint8)


def _sure(subx, suby, rows, cols, eps):
    """(surely EASU interior, surely border band or background) masks of a coordinate field"""
    sx = np.trunc(np.clip(subx, -2e9, 2e9)).astype(np.int64); sy = np.trunc(np.clip(suby, -2e9, 2e9)).astype(np.int64)
    border = (sx < 1) | (sy < 1) | (sx >= cols - 4) | (sy >= rows - 4)
    near = (np.abs(subx - np.rint(subx)) < eps) | (np.abs(suby - np.rint(suby)) < eps)
    return ~border & ~near, border & ~near


class Tally:
    """the differing-byte share is a property of a set of cases (one size, one texture): a 67 x 131 frame has 26 331 bytes, of which 1e-4 are 2.6"""
    def __init__(self):
        self.total = self.differing = 0

    def check(self, got, want, untouched, what):
        got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        print(f"{what}: max |diff| {int(d.max())}, {int((d != 0).sum())} of {d.size} bytes differ")
        assert d.max() <= 1, f"{what}: max |diff| {int(d.max())}"
        if untouched is not None:
            assert not untouched.all(), what
            assert not d[untouched].any(), f"{what}: {int((d[untouched] != 0).sum())} border-band / background bytes differ"
        self.total += d.size; self.differing += int((d != 0).sum())

    def close(self, what):
        print(f"{what}: {self.differing} of {self.total} bytes differ ({self.differing / max(self.total, 1):.2e})")
        assert self.differing <= MAX_SHARE * self.total, f"{what}: {self.differing} of {self.total} bytes differ"


def _exact(got, want, what):
    got = got.cpu().numpy()
    assert np.array_equal(got, want), f"{what}: back in EXACT mode {int((got != want).sum())} bytes differ from the oracle"


def _both_modes(pctx, run, want, untouched, tally, what):
    """run() in 1LSB mode against the bounds, then in EXACT mode against the oracle bit for bit"""
    pctx.set_remap_precision("1lsb")
    try:
        assert pctx.remap_precision == 1
        got = run(); pctx.sync()
        outs = got if isinstance(got, (tuple, list)) else [got]
        for k, (g, w) in enumerate(zip(outs, want if isinstance(want, (tuple, list)) else [want])):
            tally.check(g, w, untouched[k] if isinstance(untouched, (tuple, list)) else untouched, f"{what}[{k}]")
    finally:
        pctx.set_remap_precision("exact")
    assert pctx.remap_precision == 0
    got = run(); pctx.sync()
    for k, (g, w) in enumerate(zip(got if isinstance(got, (tuple, list)) else [got], want if isinstance(want, (tuple, list)) else [want])):
        _exact(g, w, f"{what}[{k}]")


def _homographies(rows, cols):
    cx, cy = (cols - 1) / 2.0, (rows - 1) / 2.0
    th = 0.5; c, s = np.cos(th), np.sin(th)
    degenerate = np.array([[c, -s, cx - c * cx + s * cy + 0.45 * cols], [s, c, cy - s * cx - c * cy + 0.3 * rows], [0, 0, 1]])
    perspective = np.array([[1.012, 0.021, -1.7], [-0.017, 0.991, 2.3], [2.1e-5, -1.6e-5, 1.0]])
    return {"perspective": perspective.astype(f32), "degenerate": degenerate.astype(f32)}


def _mesh(mr, mc, rows, cols):
    """random offsets; the top-left vertices carry that corner's source out of the frame (background)"""
    m = synth.random_mesh(mr, mc, np.random.default_rng(mr * 100 + rows), amp=0.03)
    m[:max(mr // 4, 1), :max(mc // 4, 1)] = (-0.3, -0.25)
    return m.astype(f32)


def _mesh_coords(oracle, mesh, rows, cols):
    if mesh.shape[:2] == (2, 2):
        return np_easu_1lsb.homography_coords(rows, cols, oracle.mesh2x2_to_homography(mesh, rows, cols))
    yy, xx = np.mgrid[0:rows, 0:cols]
    m = oracle.mesh_to_map(mesh, rows, cols)
    return xx.astype(f32) + m[..., 0], yy.astype(f32) + m[..., 1]


def _lens_coords(oracle, u, v, params, rows, cols):
    """the fused coordinate through the oracle's materialised lens map (the kernel evaluates it in closed form)"""
    lmap = oracle.lens_offset_map(params, rows, cols)[0]
    ui = np.trunc(np.clip(u, -2e9, 2e9)).astype(np.int64); vi = np.trunc(np.clip(v, -2e9, 2e9)).astype(np.int64)
    ok = (ui >= 0) & (ui < cols) & (vi >= 0) & (vi < rows)
    uc, vc = np.clip(ui, 0, cols - 1), np.clip(vi, 0, rows - 1)
    return np.where(ok, u + lmap[vc, uc, 0], f32(-16)), np.where(ok, v + lmap[vc, uc, 1], f32(-16))


def _untouched3(subx, suby, rows, cols, eps, what):
    ea, rest = _sure(subx, suby, rows, cols, eps)
    assert ea.sum() > 0.2 * ea.size and rest.sum() > 0, (what, int(ea.sum()), int(rest.sum()))
    return np.repeat(rest[..., None], 3, axis=2)


@pytest.mark.parametrize("texture", ["noise", "sinusoid_noise"])
@pytest.mark.parametrize("size", SIZES)
def test_packed_kernels_both_programs(pctx, oracle, size, texture):
    """homography (perspective, degenerate), mesh 16 x 16 (LDS) and 33 x 33 (> 2 048 values: global memory), a materialised map, the lens variants"""
    rows, cols = size
    src = _texture(texture, rows, cols); d = _gpu(src)
    yy, xx = np.mgrid[0:rows, 0:cols]
    params = LENS(rows, cols)
    tally = Tally()
    for yuv in (True, False):
        for name, H in _homographies(rows, cols).items():
            subx, suby = np_easu_1lsb.homography_coords(rows, cols, H)
            what = f"homography {name} yuv={int(yuv)} {size} {texture}"
            _both_modes(pctx, lambda: pctx.remap_homography(d, H, bg=BG, yuv=yuv), oracle.remap_homography(src, H, bg=BG, yuv=yuv),
                        _untouched3(subx, suby, rows, cols, 2e-3, what), tally, what)
            if name == "degenerate":
                sx = np.trunc(subx); sy = np.trunc(suby)
                assert ((sx < 0) | (sy < 0) | (sx >= cols) | (sy >= rows)).mean() > 0.05, "part of the frame must be background"
                m = np.stack([subx - xx.astype(f32), suby - yy.astype(f32)], -1).astype(f32); dm = _gpu(m)
                what = f"map yuv={int(yuv)} {size} {texture}"
                _both_modes(pctx, lambda: pctx.remap_map(d, dm, bg=BG, yuv=yuv), oracle.remap_map(src, m, bg=BG, yuv=yuv),
                            _untouched3(xx.astype(f32) + m[..., 0], yy.astype(f32) + m[..., 1], rows, cols, 2e-3, what), tally, what)
        for mr in (2, 16, 33):
            mesh = _mesh(mr, mr, rows, cols)
            assert (mr * mr * 2 > 2048) == (mr == 33)
            u, v = _mesh_coords(oracle, mesh, rows, cols)
            what = f"warpmesh_apply {mr}x{mr} yuv={int(yuv)} {size} {texture}"
            _both_modes(pctx, lambda: pctx.warpmesh_apply(d, mesh, bg=BG, yuv=yuv), oracle.warpmesh_apply(src, mesh, bg=BG, yuv=yuv),
                        _untouched3(u, v, rows, cols, 2e-3, what), tally, what)
            if mr != 33:
                what = f"warpmesh_apply_lens {mr}x{mr} yuv={int(yuv)} {size} {texture}"
                _both_modes(pctx, lambda: pctx.warpmesh_apply_lens(d, mesh, params, bg=BG, yuv=yuv), oracle.warpmesh_apply_lens(src, mesh, params, bg=BG, yuv=yuv),
                            _untouched3(*_lens_coords(oracle, u, v, params, rows, cols), rows, cols, 0.05, what), tally, what)
        mesh = _mesh(16, 16, rows, cols)                     # the mesh kernel proper (lvk_hip_remap_mesh takes no homography route)
        what = f"remap_mesh 16x16 yuv={int(yuv)} {size} {texture}"
        _both_modes(pctx, lambda: pctx.remap_mesh(d, mesh, bg=BG, yuv=yuv), oracle.remap_mesh(src, mesh, bg=BG, yuv=yuv),
                    _untouched3(*_mesh_coords(oracle, mesh, rows, cols), rows, cols, 2e-3, what), tally, what)
    tally.close(f"packed kernels {size} {texture}")


def _untouched420(rest, nv12):
    """luma: per pixel; a chroma sample is untouched when all four pixels under it are"""
    c = rest[0::2, 0::2] & rest[0::2, 1::2] & rest[1::2, 0::2] & rest[1::2, 1::2]
    return (rest, np.repeat(c[..., None], 2, axis=2)) if nv12 else (rest, c, c)


@pytest.mark.parametrize("texture", ["noise", "sinusoid_noise"])
@pytest.mark.parametrize("size", SIZES_EVEN)
def test_fused_420_sinks(pctx, oracle, size, texture):
    rows, cols = size
    src = _texture(texture, rows, cols); d = _gpu(src)
    tally = Tally()
    for mr in (2, 16, 33):
        mesh = _mesh(mr, mr, rows, cols)
        ea, rest = _sure(*_mesh_coords(oracle, mesh, rows, cols), rows, cols, 2e-3)
        assert ea.sum() > 0.2 * ea.size and rest.sum() > 0
        packed = oracle.warpmesh_apply(src, mesh, bg=BG, yuv=True)
        for nv12 in (False, True):
            _both_modes(pctx, lambda: pctx.warpmesh_apply_yuv420(d, mesh, bg=BG, nv12=nv12), oracle.egress_yuv420(packed, nv12=nv12),
                        _untouched420(rest, nv12), tally, f"{'NV12' if nv12 else 'I420'} {mr}x{mr} {size} {texture}")
    tally.close(f"4:2:0 sinks {size} {texture}")


def _untouched_obs(fmt, rest):
    if fmt == "I444":
        return [rest, rest, rest]
    pair = rest[:, 0::2] & rest[:, 1::2]                     # UYVY: (U, Y0, V, Y1) per pixel pair
    out = np.zeros(rest.shape + (2,), bool)
    out[..., 1] = rest
    out[:, 0::2, 0] = pair; out[:, 1::2, 0] = pair
    return [out]


@pytest.mark.parametrize("fmt", ["UYVY", "I444"])
@pytest.mark.parametrize("size", SIZES_EVEN)
def test_fused_obs_sinks(pctx, oracle, size, fmt):
    """The sinks of remap_obs.hip are reached through lvk_hip_stab_push_obs only: a short stream through a stabilizer in 1LSB mode, each emitted frame against
    the oracle stabilizer's (the correction the oracle applied gives the coordinates), then the same stream through an EXACT stabilizer bit for bit."""
    import livevisionkit_amd as lvk
    rows, cols = size
    n, delay = 7, 2
    clip, _ = synth.make_clip(rows, cols, n, seed=31, jitter=1.0)
    so = oracle_lib.preset("homography", predictive_samples=delay, min_scene_quality=0.0, min_tracking_quality=0.0)
    sg = lvk.StabilizationFilterSettings()
    ctypes.memmove(ctypes.byref(sg), ctypes.byref(so), ctypes.sizeof(so))
    ffmt = pctx.obs_frame_format(fmt)
    bg = tuple(int(so.background[i]) for i in range(3))
    ost = oracle_lib.OracleStabilizer(oracle, so)
    want = {}
    for i, f in enumerate(clip):
        planes = oracle.egress_obs(fmt, f)
        w, wts = ost.push(oracle.ingest_obs(fmt, planes), ts=i, fmt=ffmt)
        if w is not None:
            mesh = ost.meshes()[1]
            assert np.array_equal(w, oracle.warpmesh_apply(oracle.ingest_obs(fmt, oracle.egress_obs(fmt, clip[wts])), mesh, bg=bg, yuv=True))
            ea, rest = _sure(*_mesh_coords(oracle, mesh, rows, cols), rows, cols, 2e-3)      # (at 270 x 480 the stable-region crop keeps every pixel interior)
            assert ea.sum() > 0.2 * ea.size and (rest.sum() > 0 or rows > 66)
            want[wts] = (oracle.egress_obs(fmt, w), _untouched_obs(fmt, rest))
    ost.close()
    assert sorted(want) == list(range(n - delay))
    for precision in ("1lsb", "exact"):
        gst = lvk.StabilizationFilter(sg, context=pctx)
        gst.set_remap_precision(precision)
        tally = Tally()
        for i, f in enumerate(clip):
            got, ts = gst.apply_obs(fmt, [_gpu(p) for p in oracle.egress_obs(fmt, f)], timestamp=i)
            pctx.sync()
            assert (got is not None) == (i >= delay)
            if got is not None:
                for k, g in enumerate(got):
                    if precision == "exact":
                        _exact(g, want[ts][0][k], f"{fmt} {size} frame {ts} plane {k}")
                    else:
                        tally.check(g, want[ts][0][k], want[ts][1][k], f"{fmt} {size} frame {ts} plane {k}")
        if precision == "1lsb":
            tally.close(f"{fmt} {size}")
        gst.close()


def test_uncovered_entries_stay_exact_in_one_lsb_mode(pctx, oracle):
    """lvk_hip_upscale and the one-channel remaps have no 1-LSB kernels: byte-identical to the oracle with the context in 1LSB mode"""
    rows, cols = 67, 131
    src = _texture("noise", rows, cols); d = _gpu(src)
    g3 = np.full((rows, cols, 3), 128, np.uint8); g3[..., 0] = src[..., 0]
    dg = _gpu(src[..., 0])
    H = _homographies(rows, cols)["perspective"]
    mesh = _mesh(16, 16, rows, cols)
    pctx.set_remap_precision("1lsb")
    try:
        for yuv in (True, False):
            got = pctx.upscale(d, (197, 101), yuv=yuv); pctx.sync()
            _exact(got, oracle.upscale(src, (197, 101), yuv=yuv), f"upscale yuv={int(yuv)}")
        got = pctx.remap_homography_gray(dg, H, bg=BG[0]); pctx.sync()
        _exact(got, oracle.remap_homography(g3, H, bg=BG, yuv=False)[..., 0], "remap_homography_gray")
        got = pctx.warpmesh_apply_gray(dg, mesh, bg=BG[0]); pctx.sync()
        _exact(got, oracle.warpmesh_apply(g3, mesh, bg=BG, yuv=False)[..., 0], "warpmesh_apply_gray")
    finally:
        pctx.set_remap_precision("exact")


def test_unknown_precision_is_refused_and_changes_nothing(pctx):
    from livevisionkit_amd.context import LvkHipError
    lib = pctx.lib
    assert lib.lvk_hip_get_remap_precision(pctx.handle) == 0
    assert lib.lvk_hip_set_remap_precision(pctx.handle, 1) == 0
    for bad in (2, -1, 255):
        assert lib.lvk_hip_set_remap_precision(pctx.handle, bad) == -1
        assert b"precision" in lib.lvk_hip_last_error(pctx.handle)
        assert lib.lvk_hip_get_remap_precision(pctx.handle) == 1
    with pytest.raises(LvkHipError):
        pctx.set_remap_precision("sloppy")
    assert pctx.remap_precision == 1
    assert lib.lvk_hip_set_remap_precision(pctx.handle, 0) == 0 and pctx.remap_precision == 0
