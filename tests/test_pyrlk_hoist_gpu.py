"""k_pyrlk with the Newton iteration's loop-invariant operands in registers (patch samples, window offsets) and 32-bit row partials:
positions and status bit-equal to oracle.pyrlk through the synchronous flow entry, on small frames chosen so that every property the
hoisted form depends on is exercised -- and checked on the CPU to be exercised, with a model of the tracker (tests/np_pyrlk.py's
arithmetic) that records what each point's iterations do:

* both window trips (pixels 0..63 and 64..120 of the 11 x 11 window): points whose gradient lies in the last 57 pixels alone;
* the window of the next frame re-staged in the middle of a level (the LDS writes that keep the compiler from hoisting): tracks that
  leave the LK_MARGIN = 8 pixel search margin, at the first iteration of a level and at a later one;
* the 32-bit partial sums of a 16-lane DPP row at their largest: a black / white checkerboard against its inverse;
* reflect-101 staging at the frame border, levels skipped because the point lies outside or the system is singular.

No point is left out of a comparison and no tolerance is applied; every case's oracle status is 1 for at least 90 % of its points."""
import functools

import numpy as np
import pytest

from tests import np_pyrlk
from tests.clipgen import Clip

pytestmark = pytest.mark.gpu

WIN = 11
LK_MARGIN = 8                       # csrc/pyrlk.hip
FULL = 8160 * 4080                  # |diff| <= 255 * 32, |Ix|, |Iy| <= 16 * 255: the largest term of a mismatch sum


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _equal(ctx, oracle, prev, nxt, pts, n=None, min_ok=0.9):
    """GPU == oracle for the first n points, bit for bit, all of them; the oracle tracks at least min_ok of them."""
    want_p, want_s = oracle.pyrlk(prev, nxt, pts)
    n = len(pts) if n is None else n
    assert want_s[:n].mean() >= min_ok, f"oracle status 1 for {want_s[:n].mean():.2%} only"
    got_p, got_s = ctx.pyrlk(_gpu(prev), _gpu(nxt), pts[:n])
    assert got_p.shape == (n, 2) and got_s.shape == (n,)
    assert np.array_equal(got_s, want_s[:n])
    assert np.array_equal(got_p.view(np.uint32), want_p[:n].view(np.uint32)), np.abs(got_p - want_p[:n]).max()


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _textured_pair(rows, cols, tx, ty, deg, band=None, faint=None):
    """Two luma frames of the clip generator's scene: the second is the first moved by (tx, ty) pixels and rotated by deg about the centre.
    band = (y0, y1): those rows of the scene are flat (128).  faint = (y0, y1): those rows carry a +-4 checker of 2 x 2 cells on 128
    instead, which the pyramid's 5 x 5 filter brings below half a grey level (coarser levels are flat and singular there, level 0 is not)."""
    clip = Clip(rows, cols, 2, seed=rows * 1000 + cols)
    m = clip.m
    if band:
        clip.canvases[0][0][m + band[0]:m + band[1]] = 128.0
    if faint:
        H, W = clip.canvases[0][0].shape
        yy, xx = np.mgrid[0:H, 0:W]
        import torch
        chk = torch.from_numpy((128.0 + 4.0 * ((((yy >> 1) + (xx >> 1)) & 1) * 2 - 1)).astype(np.float32))
        clip.canvases[0][0][m + faint[0]:m + faint[1]] = chk[m + faint[0]:m + faint[1]]
    clip.shaky[0] = (0.0, 0.0, 0.0, 0.0)
    clip.shaky[1] = (-tx, -ty, np.deg2rad(deg), 0.0)
    f = [np.ascontiguousarray(clip.render444(i).numpy()[..., 0]) for i in (0, 1)]
    return f[0], f[1]


def _random_points(rows, cols, n, seed, margin=6.0):
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(margin, cols - margin, n), rng.uniform(margin, rows - margin, n)].astype(np.float32)


def _checkerboard(rows, cols, cell, x0=0, y0=0):
    yy, xx = np.mgrid[0:rows, 0:cols]
    return (((((yy + y0) // cell) + ((xx + x0) // cell)) & 1) * 255).astype(np.uint8)


# ---- a model of the tracker that records what the iterations do --------------------------------------------------------------------

def _trace(prev, nxt, pts, max_level=3, max_count=5, epsilon=0.01, min_eig=1e-4):
    """np_pyrlk.calc with its window arithmetic, point by point, plus a record per point: the largest |partial sum| of a 16-lane DPP row
    (lane l holds window pixels l and l + 64; a row is lanes 16 r .. 16 r + 15), the (level, iteration) pairs at which the kernel
    re-stages the next-frame window (the position's window leaves the one staged around the level's zero-flow prediction, or around the
    last re-staging), the levels skipped, and at level 0 whether the first 64 / the last 57 window pixels carry any gradient."""
    f32 = np_pyrlk.f32
    win = (WIN, WIN)
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    P, N = np_pyrlk.build_pyramid(prev, max_level, win), np_pyrlk.build_pyramid(nxt, max_level, win)
    half = f32((WIN - 1) * 0.5)
    pad = WIN + 2
    lane_row = (np.arange(WIN * WIN) % 64) // 16
    recs = []
    out_all = np.zeros((len(pts), 2), np.float32); st_all = np.ones(len(pts), np.uint8)
    planes = []
    for level in range(len(P)):
        dx_, dy_ = np_pyrlk.scharr(P[level])
        planes.append((np.pad(P[level].astype(np.int64), pad, mode="reflect"), np.pad(dx_, pad, mode="constant"),
                       np.pad(dy_, pad, mode="constant"), np.pad(N[level].astype(np.int64), pad, mode="reflect")))
    for i, p in enumerate(pts):
        rec = {"row_max": 0, "restage": [], "skipped": [], "trip1": False, "trip2": False}
        out = np.zeros(2, np.float32)
        for level in range(len(P) - 1, -1, -1):
            I, Ix, Iy, J = planes[level]
            rows, cols = P[level].shape
            inv = f32(1.0 / (1 << level))
            px, py = f32(p[0] * inv), f32(p[1] * inv)
            nx, ny = (px, py) if level == len(P) - 1 else (f32(out[0] * f32(2.0)), f32(out[1] * f32(2.0)))
            out[:] = (nx, ny)
            jx0, jy0 = int(np.floor(f32(px - half))) - LK_MARGIN, int(np.floor(f32(py - half))) - LK_MARGIN
            px, py = f32(px - half), f32(py - half)
            ipx, ipy = int(np.floor(px)), int(np.floor(py))
            if ipx < -WIN or ipx >= cols or ipy < -WIN or ipy >= rows:
                rec["skipped"].append(level)
                if level == 0:
                    st_all[i] = 0
                continue
            w = np_pyrlk._weights(f32(px - f32(ipx)), f32(py - f32(ipy)))
            Iw = np_pyrlk._sample(np_pyrlk._window(I, pad, ipy, ipx, win), w, 9)
            Ixw = np_pyrlk._sample(np_pyrlk._window(Ix, pad, ipy, ipx, win), w, 14)
            Iyw = np_pyrlk._sample(np_pyrlk._window(Iy, pad, ipy, ipx, win), w, 14)
            A11 = f32(f32(int((Ixw * Ixw).sum())) * np_pyrlk.FLT_SCALE); A12 = f32(f32(int((Ixw * Iyw).sum())) * np_pyrlk.FLT_SCALE)
            A22 = f32(f32(int((Iyw * Iyw).sum())) * np_pyrlk.FLT_SCALE)
            D = f32(f32(A11 * A22) - f32(A12 * A12)); d = f32(A11 - A22)
            min_e = f32(f32(f32(A22 + A11) - np.sqrt(f32(f32(d * d) + f32(f32(f32(4.0) * A12) * A12)))) / f32(2 * WIN * WIN))
            if min_e < f32(min_eig) or D < np_pyrlk.FLT_EPSILON:
                rec["skipped"].append(level)
                if level == 0:
                    st_all[i] = 0
                continue
            if level == 0:
                g = (np.abs(Ixw) + np.abs(Iyw)).ravel()
                rec["trip1"], rec["trip2"] = bool(g[:64].any()), bool(g[64:].any())
            D = f32(f32(1.0) / D)
            nx, ny = f32(nx - half), f32(ny - half)
            pdx = pdy = f32(0.0)
            for j in range(max_count):
                inx, iny = int(np.floor(nx)), int(np.floor(ny))
                if inx < -WIN or inx >= cols or iny < -WIN or iny >= rows:
                    if level == 0:
                        st_all[i] = 0
                    break
                if inx < jx0 or iny < jy0 or inx > jx0 + 2 * LK_MARGIN or iny > jy0 + 2 * LK_MARGIN:
                    rec["restage"].append((level, j))
                    jx0, jy0 = inx - LK_MARGIN, iny - LK_MARGIN
                wj = np_pyrlk._weights(f32(nx - f32(inx)), f32(ny - f32(iny)))
                diff = np_pyrlk._sample(np_pyrlk._window(J, pad, iny, inx, win), wj, 9) - Iw
                assert np.abs(diff).max() <= 8160 and max(np.abs(Ixw).max(), np.abs(Iyw).max()) <= 4080
                for prod in ((diff * Ixw).ravel(), (diff * Iyw).ravel()):
                    rec["row_max"] = max(rec["row_max"], int(np.abs(np.bincount(lane_row, weights=prod.astype(np.float64), minlength=4)).max()))
                b1 = f32(f32(int((diff * Ixw).sum())) * np_pyrlk.FLT_SCALE); b2 = f32(f32(int((diff * Iyw).sum())) * np_pyrlk.FLT_SCALE)
                dx = f32(f32(f32(A12 * b2) - f32(A22 * b1)) * D); dy = f32(f32(f32(A12 * b1) - f32(A11 * b2)) * D)
                nx, ny = f32(nx + dx), f32(ny + dy)
                out[:] = (f32(nx + half), f32(ny + half))
                if float(dx) * float(dx) + float(dy) * float(dy) <= epsilon * epsilon:
                    break
                if j > 0 and abs(float(f32(dx + pdx))) < 0.01 and abs(float(f32(dy + pdy))) < 0.01:
                    out[:] = (f32(out[0] - f32(dx * f32(0.5))), f32(out[1] - f32(dy * f32(0.5))))
                    break
                pdx, pdy = dx, dy
        out_all[i] = out
        recs.append(rec)
    return out_all, st_all, recs


def _traced(oracle, prev, nxt, pts):
    """The records of _trace, after checking that the model walked the oracle's own path (same positions and status, bit for bit)."""
    want_p, want_s = oracle.pyrlk(prev, nxt, pts)
    got_p, got_s, recs = _trace(prev, nxt, pts)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
    return recs


# ---- the cases ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 600])
@pytest.mark.parametrize("rows,cols", [(64, 96), (90, 160)])
def test_point_counts_on_generator_texture(ctx, oracle, rows, cols, n):
    """Sub-pixel shift plus a small rotation; the first n of one set of 600 points (a point's result does not depend on the others)."""
    prev, nxt = _textured_pair(rows, cols, 1.3, -0.7, 0.4)
    _equal(ctx, oracle, prev, nxt, _random_points(rows, cols, 600, seed=rows), n=n)


def test_gradient_in_the_second_trip_alone(ctx, oracle):
    """Rows 0 .. 29 of the scene are flat: a point at an integer position (weights 1, 0, 0, 0) in row 24 or 25 has zero derivatives in
    the window rows above scene row 29, i.e. in all of window pixels 0 .. 63, and texture below.  The mirrored points (texture above a flat
    band) have their gradient in the first trip.  A second trip that contributed nothing, or garbage from a masked lane, cannot pass."""
    rows, cols = 64, 96
    prev, nxt = _textured_pair(rows, cols, 0.6, 0.4, 0.0, band=(0, 30))
    xs = np.arange(8, cols - 8, 3, dtype=np.float32)
    pts = np.concatenate([np.c_[xs, np.full_like(xs, 24.0)], np.c_[xs, np.full_like(xs, 25.0)]]).astype(np.float32)
    recs = _traced(oracle, prev, nxt, pts)
    second_only = [r for r in recs if r["trip2"] and not r["trip1"]]
    assert len(second_only) >= len(pts) // 2, len(second_only)
    _equal(ctx, oracle, prev, nxt, pts)


def test_window_restaged_mid_level(ctx, oracle):
    """A displacement beyond the 8-pixel search margin: the level's window of the next frame is staged again inside the iteration loop, at
    the first iteration (the start, twice the coarser level's result, is already outside) and at later ones (the track walks out).  The
    patch registers loaded before the loop must survive it."""
    rows, cols = 90, 160
    prev, nxt = _textured_pair(rows, cols, 11.4, -9.3, 0.6)
    pts = _random_points(rows, cols, 200, seed=5, margin=14.0)
    recs = _traced(oracle, prev, nxt, pts)
    assert sum(1 for r in recs if (0, 0) in r["restage"]) >= 100
    assert sum(1 for r in recs if any(j > 0 for _, j in r["restage"])) >= 1
    _equal(ctx, oracle, prev, nxt, pts)


def test_row_partials_at_their_largest(ctx, oracle):
    """Black / white checkerboards against their inverses: |diff| = 8160 wherever the window is sampled at integer positions, |Ix| / |Iy|
    up to 4080 along the cell edges.  The model gives the largest |partial| of any DPP row over every iteration of every point and level
    (547 291 200 = 2^29.03 = 16.4 full-scale terms 8160 x 4080 when this was written).  It must stay below 2^31: the claim the 32-bit in-row
    steps rest on, whose a-priori bound is 32 terms x 8160 x 4080 = 1.07e9.  And it must reach at least 8 full-scale terms, a quarter of a
    row's 32, so that the case is known to press on the bound.  (All 32 cannot be asked for: with J = 255 - I the products of consecutive
    window rows, s(y) (s(y - 1) - s(y + 1)) / 2 for s = +-1, telescope, so full-scale rows of one sign never lie next to each other.)
    Cell sizes and phases are those for which the oracle still reports status 1 for 90 % of the points."""
    rows, cols = 64, 96
    cases = []
    for cell, x0, y0 in [(3, 0, 0), (3, 1, 2), (4, 0, 0), (7, 3, 3)]:
        prev = _checkerboard(rows, cols, cell, x0, y0)
        cases.append((prev, (255 - prev).astype(np.uint8)))
    yy, xx = np.mgrid[10:rows - 10:4, 10:cols - 10:5]
    pts = np.c_[xx.ravel(), yy.ravel()].astype(np.float32)
    worst = 0
    for prev, nxt in cases:
        recs = _traced(oracle, prev, nxt, pts)
        worst = max(worst, max(r["row_max"] for r in recs))
    print("largest DPP row partial: %d = 2^%.2f = %.1f full-scale terms" % (worst, np.log2(max(worst, 1)), worst / FULL))
    assert 2 * 16 * FULL < 2 ** 31
    assert worst < 2 ** 31
    assert worst >= 8 * FULL
    for prev, nxt in cases:
        _equal(ctx, oracle, prev, nxt, pts)


def test_border_and_skipped_levels(ctx, oracle):
    """Points on and just beyond the frame border (reflect-101 staging of both windows), points outside (every level or level 0 alone is
    skipped), and points on a faint fine checker that the pyramid averages away: their coarser levels are singular and skipped, level 0
    tracks."""
    rows, cols = 90, 160
    prev, nxt = _textured_pair(rows, cols, 0.8, -1.1, 0.3, faint=(40, 90))
    rng = np.random.default_rng(9)
    edge = []
    for _ in range(40):
        x, y = rng.uniform(0, cols), rng.uniform(0, 36)
        side = rng.integers(0, 3)
        edge.append([(rng.uniform(-4.5, 2.0), y), (rng.uniform(cols - 3.0, cols + 3.5), y), (x, rng.uniform(-4.5, 2.0))][side])
    outside = [(-8.0, 20.0), (-30.0, 30.0), (cols + 9.0, 40.0), (50.0, -7.5)]
    faint = [(x, y) for y in (70.0, 73.0, 76.5, 79.0, 81.25) for x in np.arange(12.0, cols - 12.0, 9.5)]
    pts = np.array(edge + outside + faint, np.float32)
    recs = _traced(oracle, prev, nxt, pts)
    assert sum(1 for r in recs if r["skipped"] and 0 not in r["skipped"]) >= 10          # coarser levels skipped, level 0 tracked
    assert sum(1 for r in recs if 0 in r["skipped"]) >= len(outside)
    _equal(ctx, oracle, prev, nxt, pts, min_ok=0.9)
