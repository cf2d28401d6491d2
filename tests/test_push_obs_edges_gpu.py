"""lvk_hip_stab_push_obs / lvk_hip_stab_push_yuv420 at the edges of the push state machine, enumerated (nothing here is random) against the oracle's
ingest -> StabilizationFilter -> egress of the same planes:

  A. a frame size that changes three times mid-stream (shrink, grow past the first size, back to it) for every format class, overlap on / off,
     stabilize_output on / off -- every pool slot is recycled after each change; the output planes sit inside guard rows and guard bytes;
  B. a switch of the format CLASS (BGR / RGB against YUV) while frames are queued is refused before anything changes, and restart() recovers;
     switches inside one class stay accepted and bit-exact;
  C. malformed planes (a NULL chroma plane, a short step, an odd width, a zero or negative size, Y800) are refused before anything changes, and the
     stream carries on as if the refused push had never been made;
  D. the fused remap + egress sinks write padded, unaligned output planes (a partial last pixel strip) and not one byte outside the frame.

Every malformed argument of C points into an allocation that holds the geometry it claims: a library that failed to refuse one reads only
allocated bytes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QA = dict(predictive_samples=3, min_scene_quality=0.3, min_tracking_quality=0.2)
GUARD = 0xA5
DIRECT4 = ("RGBA", "BGRA", "BGRX")                           # DirectIngest's 4-byte formats: tight rows (FrameIngest.cpp:743-753)
OBS_FORMATS = ["I420", "NV12", "YVYU", "YUY2", "UYVY", "RGBA", "BGRA", "BGRX", "I444", "BGR3", "I422", "I40A", "I42A", "YUVA", "AYUV"]
FORMAT_NAMES = {0: "BGR", 2: "RGB", 4: "YUV"}


def _source(fmt, frame):
    """the frame a source of `fmt` delivers: the clip's YUV frame, or for DirectIngest's BGR / RGB formats its channels in the order U, Y, V -- a
    colour frame whose cvtColor(..2GRAY) (what the tracker sees of it) carries the clip's texture"""
    return np.ascontiguousarray(frame[..., [1, 0, 2]] if fmt in ("BGR3",) + DIRECT4 else frame)


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filters(ctx, oracle, overlap, preset="homography", stabilize=1, **qa):
    import livevisionkit_amd as lvk
    from tests import oracle_lib
    from tests.test_stabilizer_gpu import _to_settings
    s = oracle_lib.preset(preset, **dict(QA, **qa))
    s.stabilize_output = stabilize
    ost = oracle_lib.OracleStabilizer(oracle, s)
    gst = lvk.StabilizationFilter(_to_settings(s), context=ctx)
    gst.set_overlap(overlap)
    return ost, gst


def _state(gst, rows, cols, ffmt):
    """everything a refused push must leave as it was"""
    return gst.features(), gst.next_output(rows, cols, ffmt), bytes(gst.stats()), gst.schedule_counters()


def _assert_state(gst, before, rows, cols, ffmt, what):
    after = _state(gst, rows, cols, ffmt)
    assert np.array_equal(after[0], before[0]), (what, "features changed")
    assert after[1:] == before[1:], (what, "next_output / stats / schedule counters changed")


class Guarded:
    """output planes of `fmt` for a rows x cols frame, each inside its own buffer of GUARD bytes: `base` bytes in front, 8 guard rows above and
    below, `extra` bytes of pitch beyond the row (0 for DirectIngest's 4-byte formats, whose rows are tight by contract)"""

    def __init__(self, oracle, fmt, rows, cols, extra, base=0):
        import torch
        self.shapes = oracle.obs_plane_shapes(fmt, rows, cols)
        self.fmt, self.extra, self.base = fmt, extra, base
        self.flat, self.views, self.geo = [], [], []
        for sh in self.shapes:
            ch = sh[2] if len(sh) == 3 else 1
            rowb = sh[1] * ch
            pitch = rowb + extra
            off = base + 8 * pitch
            flat = torch.full((base + (sh[0] + 16) * pitch,), GUARD, dtype=torch.uint8, device="cuda")
            self.flat.append(flat)
            self.views.append(flat.as_strided(sh, (pitch, ch, 1) if len(sh) == 3 else (pitch, 1), off))
            self.geo.append((sh[0], rowb, pitch, off))

    def check(self, oracle, frame, what):
        """the planes hold FrameIngest::to_obs of `frame` (written into planes of GUARD bytes: what the reference leaves alone stays) and every
        byte outside them is still GUARD"""
        want = oracle.egress_obs(self.fmt, np.ascontiguousarray(frame), planes=[np.full(sh, GUARD, np.uint8) for sh in self.shapes])
        for i, (flat, w, (rows, rowb, pitch, off)) in enumerate(zip(self.flat, want, self.geo)):
            a = flat.cpu().numpy()
            inside = a[off:off + rows * pitch].reshape(rows, pitch)
            assert np.array_equal(inside[:, :rowb], w.reshape(rows, rowb)), (what, "plane", i, "differs from the oracle")
            assert (inside[:, rowb:] == GUARD).all(), (what, "plane", i, "written past the end of a row")
            assert (a[:off] == GUARD).all() and (a[off + rows * pitch:] == GUARD).all(), (what, "plane", i, "written outside the frame's rows")


# ---- A. frame size changes for every format class -------------------------------------------------------------------------------------------------
A_FORMATS = ["BGR3", "BGRA", "BGRX", "RGBA", "I420", "NV12", "I422", "I444", "YUY2", "UYVY", "AYUV"]
A_SIZES = [(144, 256), (112, 192), (176, 320), (144, 256)]          # shrink, grow past the first size, back to it (freed addresses come back)
A_SEGMENT = QA["predictive_samples"] + 6                            # the pool (predictive_samples + 4 slots) turns over after every change


@pytest.mark.parametrize("stabilize", [1, 0])
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("fmt", A_FORMATS)
def test_resize_every_format_class(ctx, oracle, fmt, overlap, stabilize):
    from tests import oracle_lib, synth
    big = max(r for r, _ in A_SIZES), max(c for _, c in A_SIZES)
    clip, _ = synth.make_clip(big[0], big[1], A_SEGMENT * len(A_SIZES), seed=61, jitter=1.0)
    ost, gst = _filters(ctx, oracle, overlap, stabilize=stabilize)
    ffmt = ctx.obs_frame_format(fmt)
    size_of, emitted, want_emitted = {}, 0, 0
    for i, f in enumerate(clip):
        r, c = A_SIZES[i // A_SEGMENT]
        frame = _source(fmt, f[:r, :c])
        size_of[i] = (r, c)
        planes = oracle.egress_obs(fmt, frame)
        w, wts = ost.push(oracle.ingest_obs(fmt, planes), ts=i, fmt=ffmt, out=np.zeros(big + (3,), np.uint8))
        due = gst.next_output(r, c, ffmt)
        assert (due is None) == (w is None), (fmt, i)
        out = Guarded(oracle, fmt, due[0], due[1], 0 if fmt in DIRECT4 else 32, base=5) if due else None
        dev = [_gpu(p) for p in planes]
        got, ots = gst.apply_obs(fmt, dev, timestamp=i, out=out.views if out else None)
        ctx.sync()
        assert (got is None) == (w is None), (fmt, i)
        want_emitted += w is not None
        if got is not None:
            emitted += 1
            rr, cc = size_of[wts]
            assert ots == wts and (due[0], due[1]) == (rr, cc) and gst.last_format == ffmt, (fmt, i)
            out.check(oracle, w[:rr, :cc], (fmt, i))
    assert emitted == want_emitted == len(clip) - QA["predictive_samples"]
    if stabilize:
        oracle_lib.require_live_warp(ost, f"resize {fmt}")
    ost.close(); gst.close()


# ---- B. format-class switches with frames queued ---------------------------------------------------------------------------------------------------
def _push(gst, entry, fmt, dev, ts):
    if entry == "yuv420":
        return gst.apply_yuv420(tuple(dev), timestamp=ts)
    # zeroed output planes, as the oracle's egress gets them: DirectIngest's 4-byte formats leave the last quarter of the plane alone
    import torch
    from tests import oracle_lib
    rows, cols = dev[0].shape[:2]
    due = gst.next_output(rows, cols, gst.ctx.obs_frame_format(fmt))
    out = [torch.zeros(sh, dtype=torch.uint8, device="cuda") for sh in oracle_lib.Oracle.obs_plane_shapes(fmt, due[0], due[1])] if due else None
    return gst.apply_obs(fmt, dev, timestamp=ts, out=out)


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("fa,fb,entry", [("BGR3", "I444", "obs"), ("BGR3", "I420", "obs"), ("BGR3", "I420", "yuv420"), ("I444", "BGR3", "obs"),
                                         ("UYVY", "BGRX", "obs"), ("BGRA", "RGBA", "obs"), ("RGBA", "NV12", "obs")])
def test_format_class_switch_is_refused_and_restart_recovers(ctx, oracle, fa, fb, entry, overlap):
    import livevisionkit_amd as lvk
    from tests import synth
    rows, cols, delay = 144, 256, QA["predictive_samples"]
    clip, _ = synth.make_clip(rows, cols, 2 * delay + 6, seed=67, jitter=1.0)
    ost, gst = _filters(ctx, oracle, overlap)
    fa_f, fb_f = ctx.obs_frame_format(fa), ctx.obs_frame_format(fb)
    assert fa_f != fb_f

    def step(fmt, ffmt, i):
        planes = oracle.egress_obs(fmt, _source(fmt, clip[i]))
        w, wts = ost.push(oracle.ingest_obs(fmt, planes), ts=i, fmt=ffmt)
        got, ots = _push(gst, entry if fmt == fb else "obs", fmt, [_gpu(p) for p in planes], i)
        ctx.sync()
        assert (got is None) == (w is None), (fa, fb, i)
        if w is not None:
            assert ots == wts
            for g, want in zip(got, oracle.egress_obs(fmt, w)):
                assert np.array_equal(g.cpu().numpy(), want), (fa, fb, i)
        return w is not None

    i = 0
    for _ in range(delay + 2):
        step(fa, fa_f, i); i += 1
    # the next push of format B would emit a delayed frame of format A: refused, and the caller can see it coming
    before = _state(gst, rows, cols, fb_f)
    assert before[1] == (rows, cols, fa_f)
    dev = [_gpu(p) for p in oracle.egress_obs(fb, _source(fb, clip[i]))]
    with pytest.raises(lvk.LvkHipError, match=f"queued as {FORMAT_NAMES[fa_f]} .*planes are {FORMAT_NAMES[fb_f]}"):
        _push(gst, entry, fb, dev, i)
    ctx.sync()
    _assert_state(gst, before, rows, cols, fb_f, (fa, fb))
    # restart(): the format-B stream carries on bit-exactly
    ost.restart(); gst.restart()
    emitted = sum(step(fb, fb_f, j) for j in range(i, i + delay + 3))
    assert emitted == 3
    ost.close(); gst.close()


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("formats", [("BGR3", "BGRA"), ("I420", "UYVY", "AYUV")])
def test_format_switch_within_a_class_stays_bit_exact(ctx, oracle, formats, overlap):
    """a delayed frame leaves converted to the format of the push that emits it (same class: the same packed frame)"""
    from tests import oracle_lib, synth
    rows, cols, seg = 144, 256, QA["predictive_samples"] + 3
    clip, _ = synth.make_clip(rows, cols, seg * len(formats), seed=71, jitter=1.0)
    ost, gst = _filters(ctx, oracle, overlap)
    emitted = 0
    for i, f in enumerate(clip):
        fmt = formats[i // seg]
        ffmt = ctx.obs_frame_format(fmt)
        planes = oracle.egress_obs(fmt, _source(fmt, f))
        w, wts = ost.push(oracle.ingest_obs(fmt, planes), ts=i, fmt=ffmt)
        got, ots = _push(gst, "obs", fmt, [_gpu(p) for p in planes], i)
        ctx.sync()
        assert (got is None) == (w is None), (formats, i)
        if w is not None:
            emitted += 1
            assert ots == wts
            for g, want in zip(got, oracle.egress_obs(fmt, w)):
                assert np.array_equal(g.cpu().numpy(), want), (formats, fmt, i)
    assert emitted == len(clip) - QA["predictive_samples"]
    oracle_lib.require_live_warp(ost, f"switch {formats}")
    ost.close(); gst.close()


# ---- C. malformed planes -------------------------------------------------------------------------------------------------------------------------
def _malformations(fmt, ptrs, steps, rows, cols):
    """(what, ptrs, steps, rows, cols) of every malformation of a valid rows x cols frame of `fmt` that applies to it.  Each claims no more than the
    real planes hold: a step or a width is only ever made smaller."""
    out = []
    n = 2 if fmt == "NV12" else (3 if fmt in ("I420", "I40A", "I422", "I42A", "I444", "YUVA") else 1)
    for k in range(1, n):
        p = list(ptrs); p[k] = None
        out.append((f"plane {k} NULL", p, list(steps), rows, cols))
    for k in range(n):
        s = list(steps); s[k] -= 1
        out.append((f"plane {k} step one byte short", list(ptrs), s, rows, cols))
    if fmt in ("I420", "I40A", "NV12", "I422", "I42A", "YUY2", "YVYU", "UYVY"):
        out.append(("odd cols", list(ptrs), list(steps), rows, cols - 1))
    for bad in (0, -2):
        out.append((f"rows {bad}", list(ptrs), list(steps), bad, cols))
        out.append((f"cols {bad}", list(ptrs), list(steps), rows, bad))
    return out


def _c_push_obs(gst, vf, ptrs, steps, rows, cols, ts, out):
    optr, ostep = gst.ctx._obs_args(out)
    prod = C.c_int(0); ots = C.c_uint64(0)
    return gst.lib.lvk_hip_stab_push_obs(gst.handle, vf, (C.c_void_p * 3)(*ptrs), (C.c_int * 3)(*steps), rows, cols, ts, optr, ostep, out[0].shape[0],
                                         C.byref(prod), C.byref(ots), None)


def _carry_on(ctx, oracle, ost, gst, fmt, clip, start, count, entry="obs"):
    """`count` valid pushes from clip[start]: every emitted frame equals the oracle's (which never saw a refused push)"""
    ffmt = ctx.obs_frame_format(fmt)
    emitted = 0
    for i in range(start, start + count):
        planes = oracle.egress_obs(fmt, _source(fmt, clip[i]))
        w, wts = ost.push(oracle.ingest_obs(fmt, planes), ts=i, fmt=ffmt)
        got, ots = _push(gst, entry, fmt, [_gpu(p) for p in planes], i)
        ctx.sync()
        assert (got is None) == (w is None), (fmt, i)
        if w is not None:
            emitted += 1
            assert ots == wts, (fmt, i)
            for g, want in zip(got, oracle.egress_obs(fmt, w)):
                assert np.array_equal(g.cpu().numpy(), want), (fmt, i)
    return emitted


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("fmt", OBS_FORMATS)
def test_malformed_planes_are_refused_before_anything_changes(ctx, oracle, fmt, overlap):
    import torch
    import livevisionkit_amd as lvk
    from tests import synth
    rows, cols, delay = 144, 256, QA["predictive_samples"]
    clip, _ = synth.make_clip(rows, cols, 2 * delay + 6, seed=73, jitter=1.0)
    ost, gst = _filters(ctx, oracle, overlap)
    ffmt, vf = ctx.obs_frame_format(fmt), ctx.VIDEO_FORMATS[fmt]
    i = delay + 2
    assert _carry_on(ctx, oracle, ost, gst, fmt, clip, 0, i) == 2
    # the refused pushes offer the next frame's real planes (valid output planes of the delayed frame's size); only the claimed geometry is wrong
    dev = [_gpu(p) for p in oracle.egress_obs(fmt, _source(fmt, clip[i]))]
    ptrs, steps = [p.data_ptr() for p in dev] + [None] * (3 - len(dev)), [p.stride(0) for p in dev] + [0] * (3 - len(dev))
    out = [torch.empty(sh, dtype=torch.uint8, device="cuda") for sh in oracle.obs_plane_shapes(fmt, rows, cols)]
    before = _state(gst, rows, cols, ffmt)
    assert before[1] == (rows, cols, ffmt)
    cases = _malformations(fmt, ptrs, steps, rows, cols)
    y800 = torch.zeros((rows, cols), dtype=torch.uint8, device="cuda")
    cases.append(("Y800", [y800.data_ptr(), None, None], [cols, 0, 0], rows, cols))
    for what, p, s, r, c in cases:
        v = ctx.VIDEO_FORMATS["Y800"] if what == "Y800" else vf
        rc = _c_push_obs(gst, v, p, s, r, c, i, out)
        with pytest.raises(lvk.LvkHipError):
            ctx._check(rc)
        ctx.sync()
        _assert_state(gst, before, rows, cols, ffmt, (fmt, what))
    assert _carry_on(ctx, oracle, ost, gst, fmt, clip, i, delay + 3) == delay + 3
    ost.close(); gst.close()


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("nv12", [0, 1])
def test_malformed_yuv420_planes_are_refused_before_anything_changes(ctx, oracle, nv12, overlap):
    import torch
    import livevisionkit_amd as lvk
    from tests import synth
    fmt = "NV12" if nv12 else "I420"
    rows, cols, delay = 144, 256, QA["predictive_samples"]
    clip, _ = synth.make_clip(rows, cols, 2 * delay + 6, seed=79, jitter=1.0)
    ost, gst = _filters(ctx, oracle, overlap)
    i = delay + 2
    assert _carry_on(ctx, oracle, ost, gst, fmt, clip, 0, i, entry="yuv420") == 2
    y, u, *rest = [_gpu(p) for p in oracle.egress_obs(fmt, clip[i])]
    v = u if nv12 else rest[0]
    oy = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
    ou = torch.empty((rows // 2, cols // 2, 2) if nv12 else (rows // 2, cols // 2), dtype=torch.uint8, device="cuda")
    ov = ou if nv12 else torch.empty((rows // 2, cols // 2), dtype=torch.uint8, device="cuda")
    before = _state(gst, rows, cols, 4)
    for what, c, us in (("odd cols", cols - 1, u.stride(0)), ("U step one byte short", cols, u.stride(0) - 1)):
        prod = C.c_int(0); ots = C.c_uint64(0)
        rc = gst.lib.lvk_hip_stab_push_yuv420(gst.handle, y.data_ptr(), y.stride(0), u.data_ptr(), us, v.data_ptr(), v.stride(0), nv12, rows, c, i,
                                              oy.data_ptr(), oy.stride(0), ou.data_ptr(), ou.stride(0), ov.data_ptr(), ov.stride(0), rows,
                                              C.byref(prod), C.byref(ots), None)
        with pytest.raises(lvk.LvkHipError):
            ctx._check(rc)
        ctx.sync()
        _assert_state(gst, before, rows, cols, 4, (fmt, what))
    assert _carry_on(ctx, oracle, ost, gst, fmt, clip, i, delay + 3, entry="yuv420") == delay + 3
    ost.close(); gst.close()


# ---- D. fused remap + egress sinks into padded, unaligned planes -----------------------------------------------------------------------------------
D_FORMATS = ["I422", "I42A", "YUY2", "YVYU", "UYVY", "I444", "YUVA", "AYUV", "I420", "NV12"]
D_LAYOUTS = [(0, 64), (1, 1), (3, 3)]                                # (base offset, extra pitch) of every output plane


@pytest.mark.parametrize("base,extra", D_LAYOUTS)
@pytest.mark.parametrize("fmt,preset", [(f, "homography") for f in D_FORMATS] + [(f, "field") for f in ("UYVY", "I422", "AYUV")])
def test_fused_sinks_write_padded_unaligned_planes(ctx, oracle, fmt, preset, base, extra):
    """262 columns: the last 4-pixel strip holds 2.  The remap runs on every emitted frame (stabilize_output), so every one leaves through the
    fused sink (4:2:0: the fused remap + egress kernel)."""
    from tests import oracle_lib, synth
    rows, cols, n = 144, 262, 12
    clip, _ = synth.make_clip(rows, cols, n, seed=83, jitter=1.0)
    # (the vector-field preset's local mesh keeps only a few percent of the matches as inliers at this size: with quality assurance at zero the
    #  trust factor still leaves zero, so its remaps carry the estimated mesh -- require_live_warp below)
    ost, gst = _filters(ctx, oracle, True, preset=preset, **({"min_scene_quality": 0.0, "min_tracking_quality": 0.0} if preset == "field" else {}))
    ffmt = ctx.obs_frame_format(fmt)
    emitted = 0
    for i, f in enumerate(clip):
        planes = oracle.egress_obs(fmt, f)
        w, wts = ost.push(oracle.ingest_obs(fmt, planes), ts=i, fmt=ffmt)
        out = Guarded(oracle, fmt, rows, cols, extra, base)
        got, ots = gst.apply_obs(fmt, [_gpu(p) for p in planes], timestamp=i, out=out.views)
        ctx.sync()
        assert (got is None) == (w is None), (fmt, i)
        if w is None:
            assert all((g.cpu().numpy() == GUARD).all() for g in out.flat), (fmt, i, "a push that emits nothing wrote its planes")
        else:
            emitted += 1
            assert ots == wts
            out.check(oracle, w, (fmt, preset, base, extra, i))
    assert emitted == n - QA["predictive_samples"]
    oracle_lib.require_live_warp(ost, f"fused sink {fmt} {preset}")
    ost.close(); gst.close()
