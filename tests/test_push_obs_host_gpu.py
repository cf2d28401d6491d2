"""lvk_hip_stab_push_obs_host: the host-memory entry for every OBS video format that is not 4:2:0.  lvk_hip_stab_push_obs is held to the oracle bit for
bit elsewhere (test_push_obs_edges_gpu.py, test_ingest_obs_gpu.py), so the yardstick here is BYTE EQUALITY with lvk_hip_stab_push_obs on the same frames
-- planes, timestamps, the `emitted` struct -- with no tolerance; one format of each kind also goes against the oracle directly.

Every output plane lies in a pinned block of GUARD bytes (guard bytes in front of it, behind it and behind every row); every input plane is overwritten
as soon as the push has returned.  The clips are jittered and the quality assurance is relaxed (as in test_host_frames_gpu.py), so that the trust factor
leaves zero and real homographies reach the pixels: the twin-filter test fails if it does not."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_push_obs_edges_gpu import _assert_state, _source, _state

pytestmark = pytest.mark.gpu

QA = dict(predictive_samples=3, min_scene_quality=0.3, min_tracking_quality=0.2)
DELAY = QA["predictive_samples"]
GUARD = 0xA5
PAD = 64
TIGHT = ("RGBA", "BGRA", "BGRX")                            # DirectIngest's 4-byte formats: a tight byte stream by contract
FORMATS = ["I422", "I42A", "I444", "YUVA", "YUY2", "YVYU", "UYVY", "AYUV", "BGR3", "RGBA", "BGRA", "BGRX"]
ERR_ARG = -1


@functools.lru_cache(maxsize=4)
def _clip(rows, cols, n, seed):
    from tests import synth
    return synth.make_clip(rows, cols, n, seed=seed, jitter=1.0)[0]


def _filter(ctx, overlap=True, **over):
    import livevisionkit_amd as lvk
    from tests import oracle_lib
    from tests.test_stabilizer_gpu import _to_settings
    so = oracle_lib.preset("homography", **dict(QA, **over))
    gst = lvk.StabilizationFilter(_to_settings(so), context=ctx)
    gst.set_overlap(overlap)
    return gst, so


def _shapes(fmt, rows, cols):
    from tests import oracle_lib
    return oracle_lib.Oracle.obs_plane_shapes(fmt, rows, cols)


class HostBuf:
    """the planes of one frame of `fmt` in ONE pinned block of `fill` bytes.  extra == 0: the OBS layout, the planes back to back (PAD guard bytes in
    front of the first and behind the last); extra > 0: every row `extra` bytes longer than its pixels and PAD guard bytes between the planes too."""

    def __init__(self, fmt, rows, cols, extra=0, fill=GUARD):
        import torch
        extra = 0 if fmt in TIGHT else extra
        self.geo, n = [], 0
        for sh in _shapes(fmt, rows, cols):
            ch = sh[2] if len(sh) == 3 else 1
            rowb, pitch = sh[1] * ch, sh[1] * ch + extra
            off = n + (PAD if extra or not self.geo else 0)
            n = off + sh[0] * pitch
            self.geo.append((sh, ch, rowb, pitch, off))
        n += PAD
        self.fill = fill
        self.t = torch.full((n,), fill, dtype=torch.uint8).pin_memory()
        self.a = self.t.numpy()
        as_strided = np.lib.stride_tricks.as_strided
        self.planes = [as_strided(self.a[off:], sh, (pitch, ch, 1) if len(sh) == 3 else (pitch, 1)) for sh, ch, rowb, pitch, off in self.geo]
        self.outside = np.ones(n, bool)
        for sh, ch, rowb, pitch, off in self.geo:
            as_strided(self.outside[off:], (sh[0], rowb), (pitch, 1))[...] = False

    def set(self, planes):
        for d, s in zip(self.planes, planes):
            d[...] = s

    def guards_intact(self):
        return bool((self.a[self.outside] == self.fill).all())

    def untouched(self):
        return bool((self.a == self.fill).all())


def _arrays(planes, pointer):
    """the C arrays of a plane list; a plane that is None becomes a NULL pointer with a step that is long enough for anything"""
    ptrs = (C.c_void_p * 3)(*[None if p is None else pointer(p) for p in planes] + [None] * (3 - len(planes)))
    steps = (C.c_int * 3)(*[1 << 20 if p is None else (int(p.strides[0]) if hasattr(p, "strides") else p.stride(0)) for p in planes] + [0] * (3 - len(planes)))
    return ptrs, steps


def _push(gst, entry, fmt, src, ts, dst, rows=None, cols=None):
    """one raw call of lvk_hip_stab_push_obs_host (numpy planes) / lvk_hip_stab_push_obs (torch planes): (rc, produced, timestamp, emitted)"""
    from livevisionkit_amd.stabilization import FrameInfo
    pointer = (lambda p: p.ctypes.data) if entry == "host" else (lambda p: p.data_ptr())
    ip, is_ = _arrays(src, pointer)
    op, os_ = _arrays(dst or [], pointer)
    r, c = src[0].shape[:2]
    prod = C.c_int(-5); ots = C.c_uint64(0); info = FrameInfo()
    fn = gst.lib.lvk_hip_stab_push_obs_host if entry == "host" else gst.lib.lvk_hip_stab_push_obs
    rc = fn(gst.handle, gst.ctx.VIDEO_FORMATS[fmt], ip, is_, r if rows is None else rows, c if cols is None else cols, ts, op, os_,
            dst[0].shape[0] if dst else 0, C.byref(prod), C.byref(ots), C.byref(info))
    return rc, prod.value, ots.value, (info.rows, info.cols, info.format)


def _err(ctx):
    return ctx.lib.lvk_hip_last_error(ctx.handle).decode()


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_stream(ctx, oracle, gst, frames, fmts, t0=0):
    """frames[i] (timestamp t0 + i) through lvk_hip_stab_push_obs as format fmts[i], synchronised after every push: [(timestamp, emitted, planes) or None]"""
    import torch
    res = []
    for i, f in enumerate(frames):
        fmt = fmts[i]
        rows, cols = f.shape[:2]
        dev = [_gpu(p) for p in oracle.egress_obs(fmt, _source(fmt, f))]
        due = gst.next_output(rows, cols, ctx.obs_frame_format(fmt))
        out = [torch.full(sh, GUARD, dtype=torch.uint8, device="cuda") for sh in _shapes(fmt, due[0], due[1])] if due else None
        rc, prod, ots, info = _push(gst, "dev", fmt, dev, t0 + i, out)
        ctx._check(rc)
        ctx.sync()
        assert bool(prod) == (due is not None)
        res.append((ots, info, [p.cpu().numpy() for p in out]) if prod else None)
    return res


def _host_stream(ctx, oracle, gst, frames, fmts, extra=0, sync=lambda i: True, t0=0):
    """the same frames through lvk_hip_stab_push_obs_host; the caller synchronises after push i where sync(i).  The inputs alternate between two
    pinned buffers that are overwritten as soon as the push has returned; every output has its own guarded buffer, compared after the last push."""
    res, ins = [], {}
    for i, f in enumerate(frames):
        fmt = fmts[i]
        rows, cols = f.shape[:2]
        key = (fmt, rows, cols, i % 2)
        if key not in ins:
            ins[key] = HostBuf(fmt, rows, cols, extra)
        hb = ins[key]
        hb.set(oracle.egress_obs(fmt, _source(fmt, f)))
        due = gst.next_output(rows, cols, ctx.obs_frame_format(fmt))
        out = HostBuf(fmt, due[0], due[1], extra) if due else None
        rc, prod, ots, info = _push(gst, "host", fmt, hb.planes, t0 + i, out.planes if out else None)
        ctx._check(rc)
        for p in hb.planes:
            p[...] = 99                                     # consumed on return: scribbling over the input must not matter
        if sync(i):
            ctx.sync()
        assert bool(prod) == (due is not None), (fmt, i)
        res.append((ots, info, out) if prod else None)
    ctx.sync()
    return res


def _assert_same(host, dev, what):
    assert len(host) == len(dev)
    for i, (h, d) in enumerate(zip(host, dev)):
        assert (h is None) == (d is None), (what, i, "emission differs")
        if h is None:
            continue
        assert h[0] == d[0], (what, i, "timestamp")
        if h[1] is not None:
            assert h[1] == d[1], (what, i, "emitted struct", h[1], d[1])
        for k, (a, b) in enumerate(zip(h[2].planes, d[2])):
            assert a.shape == b.shape and np.array_equal(a, b), (what, i, "plane", k, "differs from lvk_hip_stab_push_obs")
        assert h[2].guards_intact(), (what, i, "bytes outside the planes' pixels were written")


def _require_live_warp(gst, what):
    """the suite's require_live_warp rule on the filter under test: an identity warp proves nothing"""
    st = gst.stats()
    assert st.trust > 0.1, f"{what}: the trust factor ended at {st.trust:.2f}: the compared frames carry no stabilizing warp"
    motion, corr = gst.meshes()
    assert st.n_matched >= 50 and np.abs(np.asarray(motion)).max() > 0 and np.abs(np.asarray(corr)).max() > 0, f"{what}: nothing was tracked"


SCHEDULES = {"every": lambda i: True, "mixed": lambda i: i % 3 != 0, "free": lambda i: False}


# ---- twin filter: every format, contiguous and pitched planes, overlap on / off, three kinds of caller ------------------------------------------------
@pytest.mark.parametrize("extra,overlap,schedule", [(0, True, "every"), (13, False, "every"), (64, True, "mixed"), (0, False, "mixed"), (13, True, "free")])
@pytest.mark.parametrize("fmt", FORMATS)
def test_twin_filter_matches_push_obs(ctx, oracle, fmt, extra, overlap, schedule):
    n = 11
    clip = _clip(540, 960, n, 31)
    gd, _ = _filter(ctx, overlap)
    dev = _device_stream(ctx, oracle, gd, clip, [fmt] * n)
    gh, _ = _filter(ctx, overlap)
    host = _host_stream(ctx, oracle, gh, clip, [fmt] * n, extra, SCHEDULES[schedule])
    assert sum(h is not None for h in host) >= n - 3
    _assert_same(host, dev, (fmt, extra, overlap, schedule))
    _require_live_warp(gh, f"twin {fmt}")
    assert bytes(gh.stats()) == bytes(gd.stats())
    gd.close(); gh.close()


@pytest.mark.parametrize("fmt", ["I422", "UYVY", "AYUV", "BGRA"])
def test_one_format_of_each_kind_against_the_oracle(ctx, oracle, fmt):
    from tests import oracle_lib
    n = 11
    clip = _clip(540, 960, n, 31)
    gh, so = _filter(ctx, True)
    ost = oracle_lib.OracleStabilizer(oracle, so)
    host = _host_stream(ctx, oracle, gh, clip, [fmt] * n, 0, SCHEDULES["every"])
    ffmt = ctx.obs_frame_format(fmt)
    emitted = 0
    for i, f in enumerate(clip):
        w, wts = ost.push(oracle.ingest_obs(fmt, oracle.egress_obs(fmt, _source(fmt, f))), ts=i, fmt=ffmt)
        assert (w is None) == (host[i] is None), (fmt, i)
        if w is None:
            continue
        emitted += 1
        assert host[i][0] == wts and host[i][1] == (540, 960, ffmt), (fmt, i)
        want = oracle.egress_obs(fmt, w, planes=[np.full(sh, GUARD, np.uint8) for sh in _shapes(fmt, 540, 960)])
        for k, (a, b) in enumerate(zip(host[i][2].planes, want)):
            assert np.array_equal(a, b), (fmt, i, "plane", k, "differs from the oracle")
        assert host[i][2].guards_intact()
    assert emitted == n - DELAY
    oracle_lib.require_live_warp(ost, f"oracle {fmt}")
    ost.close(); gh.close()


# ---- 1080p and 4K, free running, through the Python mirror ----------------------------------------------------------------------------------------
def _planes_from_i420(fmt, y, u, v):
    """I444 / UYVY planes (torch, on the GPU) of a rendered I420 frame: the chroma samples repeated"""
    import torch
    if fmt == "I444":
        up = lambda p: p.repeat_interleave(2, 0).repeat_interleave(2, 1).contiguous()
        return [y.contiguous(), up(u), up(v)]
    rows, cols = y.shape
    out = torch.empty((rows, cols, 2), dtype=torch.uint8, device=y.device)
    out[:, :, 1] = y
    out[:, 0::2, 0] = u.repeat_interleave(2, 0)
    out[:, 1::2, 0] = v.repeat_interleave(2, 0)
    return [out]


@pytest.mark.parametrize("rows,cols", [(1080, 1920), (2160, 3840)])
@pytest.mark.parametrize("fmt", ["UYVY", "I444"])
def test_host_entry_equals_device_entry_at_1080p_and_4k(ctx, fmt, rows, cols):
    import torch
    import livevisionkit_amd as lvk
    from tests import clipgen
    n, delay = 14, 4
    clip = clipgen.Clip(rows, cols, n, device="cuda")
    planes = [_planes_from_i420(fmt, *clip.render_i420(i)) for i in range(n)]
    torch.cuda.synchronize()
    s = lvk.StabilizationFilterSettings.obs_preset("homography", strict=False, predictive_samples=delay, min_scene_quality=0.3, min_tracking_quality=0.2)

    def make():
        f = lvk.StabilizationFilter(lvk.StabilizationFilterSettings(), context=ctx); f.configure(s); f.set_overlap(True)
        return f

    gd = make()
    want = []
    for i in range(n):
        got, ts = gd.apply_obs(fmt, planes[i], timestamp=i)
        if got is not None:
            ctx.sync(); want.append((ts, [p.cpu().numpy() for p in got]))
    gh = make()
    ins = [gh.host_planes_obs(fmt, rows, cols, 64 if k else 0) for k in range(2)]            # one contiguous frame, one pitched
    ins_a = [gh.prepare_obs_host(fmt, p) for p in ins]
    outs = [gh.host_planes_obs(fmt, rows, cols) for _ in range(n)]
    outs_a = [gh.prepare_obs_host(fmt, p) for p in outs]
    host_in = [[p.cpu().numpy() for p in pl] for pl in planes]
    emitted = []
    for i in range(n):
        for d, p in zip(ins[i % 2], host_in[i]):
            d[...] = p
        got, ts = gh.apply_obs_host_prepared(ins_a[i % 2], i, outs_a[i])                      # no synchronisation between the pushes
        if got is not None:
            emitted.append((ts, i))
    ctx.sync()
    assert len(emitted) == len(want) == n - delay
    for (ts, i), (wts, wp) in zip(emitted, want):
        assert ts == wts
        for k, (a, b) in enumerate(zip(outs[i], wp)):
            assert np.array_equal(a, b), (fmt, rows, i, "plane", k)
    _require_live_warp(gh, f"{fmt} {rows}p")
    assert bytes(gh.stats()) == bytes(gd.stats())
    gd.close(); gh.close()


# ---- the smallest legal frames -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(2, 2), (1, 2)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_smallest_frames(ctx, oracle, fmt, rows, cols):
    """2 x 2, and 2 x 1 (one row of two pixels): every format here subsamples horizontally at most"""
    n = 6
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8) for _ in range(n)]
    for overlap in (False, True):
        gd, _ = _filter(ctx, overlap, predictive_samples=1)
        dev = _device_stream(ctx, oracle, gd, frames, [fmt] * n)
        gh, _ = _filter(ctx, overlap, predictive_samples=1)
        host = _host_stream(ctx, oracle, gh, frames, [fmt] * n, 0, SCHEDULES["mixed"])
        assert sum(h is not None for h in host) == n - 1
        _assert_same(host, dev, (fmt, rows, cols, overlap))
        gd.close(); gh.close()


# ---- a resize in the middle of the stream ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["UYVY", "BGRA"])
def test_mid_stream_resize(ctx, oracle, fmt):
    """540 x 960 -> 360 x 640: the next `frame_delay` outputs still have the old size; output planes of the new size are refused for them before
    anything changes, and the same push with planes of the old size succeeds"""
    n, cut = 12, 6
    clip = _clip(540, 960, n, 31)
    frames = [f if i < cut else np.ascontiguousarray(f[:360, :640]) for i, f in enumerate(clip)]
    gd, _ = _filter(ctx, True)
    dev = _device_stream(ctx, oracle, gd, frames, [fmt] * n)
    gh, _ = _filter(ctx, True)
    ffmt = ctx.obs_frame_format(fmt)
    # up to the resize, then the refusals: frames of the old size are due
    host = _host_stream(ctx, oracle, gh, frames[:cut], [fmt] * cut)
    small_in, small_out, big_out = HostBuf(fmt, 360, 640), HostBuf(fmt, 360, 640), HostBuf(fmt, 540, 960)
    for i in range(cut, n):
        small_in.set(oracle.egress_obs(fmt, _source(fmt, frames[i])))
        due = gh.next_output(360, 640, ffmt)
        old = i < cut + DELAY
        assert due == ((540, 960, ffmt) if old else (360, 640, ffmt)), i
        if old:
            before = _state(gh, 360, 640, ffmt)
            rc, prod, _, _ = _push(gh, "host", fmt, small_in.planes, i, small_out.planes)
            assert rc == ERR_ARG and prod == 0 and "do not hold the frame" in _err(ctx), i
            ctx.sync()
            _assert_state(gh, before, 360, 640, ffmt, (fmt, i))
            assert small_out.untouched()
        out = HostBuf(fmt, due[0], due[1], 0 if old else 13)
        rc, prod, ots, info = _push(gh, "host", fmt, small_in.planes, i, out.planes)
        ctx._check(rc)
        ctx.sync()
        assert prod == 1 and info == due
        host.append((ots, info, out))
    _assert_same(host, dev, ("resize", fmt))
    assert big_out.untouched()
    _require_live_warp(gh, f"resize {fmt}")
    gd.close(); gh.close()


# ---- the four entries mixed within one format class ------------------------------------------------------------------------------------------------
def test_four_entries_alternate_within_the_yuv_class(ctx, oracle):
    """push_obs (UYVY, device), push_yuv420 (I420, device), push_yuv420_host (I420, host), push_obs_host (UYVY, host), push by push: the stream
    lvk_hip_stab_push_obs alone emits for the same formats"""
    import torch
    n = 14
    clip = _clip(540, 960, n, 31)
    fmts = [("UYVY", "I420", "I420", "UYVY")[i % 4] for i in range(n)]
    gd, _ = _filter(ctx, True)
    dev = _device_stream(ctx, oracle, gd, clip, fmts)
    gm, _ = _filter(ctx, True)
    mixed = []
    for i, f in enumerate(clip):
        entry = ("obs", "yuv420", "yuv420_host", "obs_host")[i % 4]
        fmt = fmts[i]
        planes = oracle.egress_obs(fmt, f)
        out = HostBuf(fmt, 540, 960)
        if entry == "obs":
            o = [torch.full(sh, GUARD, dtype=torch.uint8, device="cuda") for sh in _shapes(fmt, 540, 960)]
            rc, prod, ots, info = _push(gm, "dev", fmt, [_gpu(p) for p in planes], i, o)
            ctx._check(rc); ctx.sync()
            out.set([p.cpu().numpy() for p in o])
        elif entry == "yuv420":
            got, ots = gm.apply_yuv420(tuple(_gpu(p) for p in planes), timestamp=i)
            ctx.sync()
            prod, info = got is not None, None
            if prod:
                out.set([p.cpu().numpy() for p in got])
        elif entry == "yuv420_host":
            src = HostBuf(fmt, 540, 960); src.set(planes)
            got, ots = gm.apply_yuv420_host_prepared(gm.prepare_yuv420_host(tuple(src.planes)), i, gm.prepare_yuv420_host(tuple(out.planes)))
            ctx.sync()
            prod, info = got is not None, None
        else:
            src = HostBuf(fmt, 540, 960); src.set(planes)
            rc, prod, ots, info = _push(gm, "host", fmt, src.planes, i, out.planes)
            ctx._check(rc); ctx.sync()
        mixed.append((ots, info, out) if prod else None)
    assert sum(m is not None for m in mixed) == n - DELAY
    _assert_same(mixed, dev, "mixed YUV entries")
    _require_live_warp(gm, "mixed entries")
    gd.close(); gm.close()


def test_device_and_host_entries_alternate_within_the_bgr_class(ctx, oracle):
    n = 12
    clip = _clip(540, 960, n, 31)
    fmts = [("BGR3", "BGRA", "BGRX", "BGR3")[i % 4] for i in range(n)]
    gd, _ = _filter(ctx, True)
    dev = _device_stream(ctx, oracle, gd, clip, fmts)
    gm, _ = _filter(ctx, True)
    mixed = []
    for i, f in enumerate(clip):
        if i % 2:
            mixed += _host_stream(ctx, oracle, gm, [f], [fmts[i]], t0=i)
        else:
            r = _device_stream(ctx, oracle, gm, [f], [fmts[i]], t0=i)[0]
            if r is not None:
                out = HostBuf(fmts[i], 540, 960); out.set(r[2])
                r = (r[0], r[1], out)
            mixed.append(r)
    assert sum(m is not None for m in mixed) == n - DELAY
    _assert_same(mixed, dev, "mixed BGR entries")
    gd.close(); gm.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
class HalfPinned:
    """a page-aligned host range of 2 * n bytes of which only the first n are registered with the runtime: every byte is allocated, the second half is
    pageable.  (hipHostRegister through torch's runtime binding.)"""

    def __init__(self, n):
        import torch
        self.n = (n + 4095) // 4096 * 4096
        self.raw = np.full(2 * self.n + 4096, GUARD, np.uint8)
        self.base = (self.raw.ctypes.data + 4095) // 4096 * 4096
        self.rt = torch.cuda.cudart()
        assert int(self.rt.cudaHostRegister(self.base, self.n, 0)) == 0
        self.view = self.raw[self.base - self.raw.ctypes.data:][:2 * self.n]

    def close(self):
        self.rt.cudaHostUnregister(self.base)


def test_refusals_leave_the_filter_as_it_was(ctx, oracle):
    rows, cols = 144, 256
    clip = _clip(rows, cols, 16, 73)
    gh, _ = _filter(ctx, True)
    fmt, ffmt = "I422", 4
    host = _host_stream(ctx, oracle, gh, clip[:DELAY + 2], [fmt] * (DELAY + 2))
    assert sum(h is not None for h in host) == 2
    i = DELAY + 2
    planes = oracle.egress_obs(fmt, clip[i])
    good_in, good_out = HostBuf(fmt, rows, cols), HostBuf(fmt, rows, cols)
    good_in.set(planes)
    uyvy_in, uyvy_out = HostBuf("UYVY", rows, cols), HostBuf("UYVY", rows, cols)
    uyvy_in.set(oracle.egress_obs("UYVY", clip[i]))
    pageable = [np.array(p) for p in planes]
    pageable_out = [np.full(sh, GUARD, np.uint8) for sh in _shapes(fmt, rows, cols)]
    # a Y plane whose first bytes are pinned and whose last rows are not
    half = HalfPinned(rows * cols // 2)
    assert 2 * half.n >= rows * cols > half.n
    straddle = half.view[:rows * cols].reshape(rows, cols)
    straddle[...] = planes[0]
    y800 = HostBuf("I444", rows, cols)                         # (three planes: more than Y800's one)
    bgr_in, bgr_out = HostBuf("BGRA", rows, cols), HostBuf("BGRA", rows, cols)
    bgr_in.set(oracle.egress_obs("BGRA", _source("BGRA", clip[i])))
    cases = [
        ("a pageable input plane", fmt, [good_in.planes[0], pageable[1], good_in.planes[2]], good_out.planes, {}, "PINNED"),
        ("all input planes pageable", fmt, pageable, good_out.planes, {}, "PINNED"),
        ("a pageable output plane", fmt, good_in.planes, [good_out.planes[0], good_out.planes[1], pageable_out[2]], {}, "PINNED"),
        ("an input plane pinned at its start only", fmt, [straddle, good_in.planes[1], good_in.planes[2]], good_out.planes, {}, "PINNED"),
        ("an output plane pinned at its start only", fmt, good_in.planes, [straddle, good_out.planes[1], good_out.planes[2]], {}, "PINNED"),
        ("a NULL chroma plane", fmt, [good_in.planes[0], None, good_in.planes[2]], good_out.planes, {}, ""),
        ("a NULL output chroma plane", fmt, good_in.planes, [good_out.planes[0], good_out.planes[1], None], {}, "do not hold the frame"),
        ("an odd width, planar 4:2:2", fmt, good_in.planes, good_out.planes, {"cols": cols - 1}, ""),
        ("an odd width, packed 4:2:2", "UYVY", uyvy_in.planes, uyvy_out.planes, {"cols": cols - 1}, ""),
        ("rows 0", "UYVY", uyvy_in.planes, uyvy_out.planes, {"rows": 0}, ""),
        ("Y800", "Y800", y800.planes[:1], y800.planes[:1], {}, "no three-channel frame"),
        ("a BGR push onto queued YUV frames", "BGRA", bgr_in.planes, bgr_out.planes, {}, "queued as YUV"),
    ]
    before = _state(gh, rows, cols, ffmt)
    assert before[1] == (rows, cols, ffmt)
    for what, f, src, dst, geo, message in cases:
        ip, is_ = _arrays(src, lambda p: p.ctypes.data)
        op, os_ = _arrays(dst, lambda p: p.ctypes.data)
        prod = C.c_int(-5); ots = C.c_uint64(0)
        rc = gh.lib.lvk_hip_stab_push_obs_host(gh.handle, ctx.VIDEO_FORMATS[f], ip, is_, geo.get("rows", rows), geo.get("cols", cols), i, op, os_, rows,
                                               C.byref(prod), C.byref(ots), None)
        assert rc == ERR_ARG and prod.value == 0, (what, rc)
        assert message in _err(ctx), (what, _err(ctx))
        ctx.sync()
        _assert_state(gh, before, rows, cols, ffmt, what)
        for b in (good_out, uyvy_out, bgr_out):
            assert b.untouched(), what
        assert (np.concatenate([p.reshape(-1) for p in pageable_out]) == GUARD).all() and (half.view[rows * cols:] == GUARD).all(), what
    # an outstanding 4:2:0 announcement: refused; after the cancel the same push goes through
    ann = gh.host_planes(rows, cols)
    for p in ann:
        p[...] = 90
    gh.prefetch_yuv420_host_prepared(gh.prepare_yuv420_host(ann))
    rc, prod, _, _ = _push(gh, "host", fmt, good_in.planes, i, good_out.planes)
    assert rc == ERR_ARG and prod == 0 and "lvk_hip_stab_prefetch_yuv420_host" in _err(ctx)
    assert good_out.untouched()
    gh.prefetch_cancel()
    ctx.sync()
    _assert_state(gh, before, rows, cols, ffmt, "announcement")
    # the stream carries on as if no refused push had been made: the twin never saw one
    gd, _ = _filter(ctx, True)
    dev = _device_stream(ctx, oracle, gd, clip, [fmt] * len(clip))
    host += _host_stream(ctx, oracle, gh, clip[i:], [fmt] * (len(clip) - i), t0=i)
    _assert_same(host, dev, "after the refusals")
    half.close()
    gd.close(); gh.close()


def test_yuv_push_onto_queued_bgr_frames_is_refused(ctx, oracle):
    rows, cols = 144, 256
    clip = _clip(rows, cols, 16, 73)
    gh, _ = _filter(ctx, True)
    _host_stream(ctx, oracle, gh, clip[:DELAY + 1], ["BGRA"] * (DELAY + 1))
    src, out = HostBuf("UYVY", rows, cols), HostBuf("UYVY", rows, cols)
    src.set(oracle.egress_obs("UYVY", clip[DELAY + 1]))
    before = _state(gh, rows, cols, 4)
    assert before[1] == (rows, cols, 0)                         # a BGR frame is due
    rc, prod, _, _ = _push(gh, "host", "UYVY", src.planes, DELAY + 1, out.planes)
    assert rc == ERR_ARG and prod == 0 and "queued as BGR" in _err(ctx)
    ctx.sync()
    _assert_state(gh, before, rows, cols, 4, "YUV onto BGR")
    assert out.untouched()
    bsrc, bout = HostBuf("BGRA", rows, cols), HostBuf("BGRA", rows, cols)
    bsrc.set(oracle.egress_obs("BGRA", _source("BGRA", clip[DELAY + 1])))
    rc, prod, ots, info = _push(gh, "host", "BGRA", bsrc.planes, DELAY + 1, bout.planes)
    ctx._check(rc); ctx.sync()
    assert prod == 1 and ots == 1 and info == (rows, cols, 0) and not bout.untouched() and bout.guards_intact()
    gh.close()


def test_the_420_delegate_refuses_what_the_420_entry_refuses(ctx, oracle):
    """I420 / I40A / NV12 are lvk_hip_stab_push_yuv420_host's: the same return codes and messages, call by call, and the same frames"""
    rows, cols = 144, 256
    clip = _clip(rows, cols, 16, 73)
    n = DELAY + 3

    def direct(gst, fmt, src, ts, dst, c=cols):
        nv12 = fmt == "NV12"
        a = lambda p: (C.c_void_p(p.ctypes.data), C.c_int(p.strides[0]))
        s, d = list(src) + ([src[1]] if nv12 else []), list(dst) + ([dst[1]] if nv12 else [])
        prod = C.c_int(-5); ots = C.c_uint64(0)
        rc = gst.lib.lvk_hip_stab_push_yuv420_host(gst.handle, *a(s[0]), *a(s[1]), *a(s[2]), int(nv12), rows, c, ts, *a(d[0]), *a(d[1]), *a(d[2]), rows,
                                                   C.byref(prod), C.byref(ots), None)
        return rc, prod.value, ots.value

    for fmt in ("I420", "NV12", "I40A"):
        ga, _ = _filter(ctx, True)
        gb, _ = _filter(ctx, True)
        for i in range(n):
            planes = oracle.egress_obs(fmt, clip[i])
            ia, ib, oa, ob = (HostBuf(fmt, rows, cols) for _ in range(4))
            ia.set(planes); ib.set(planes)
            ra = _push(ga, "host", fmt, ia.planes, i, oa.planes)
            rb = direct(gb, fmt, ib.planes, i, ob.planes)
            ctx.sync()
            assert ra[:3] == rb and ra[0] == 0, (fmt, i)
            assert np.array_equal(oa.a, ob.a) and (oa.untouched() == (i < DELAY)), (fmt, i)
        planes = oracle.egress_obs(fmt, clip[n])
        good_a, good_b, out_a, out_b = (HostBuf(fmt, rows, cols) for _ in range(4))
        good_a.set(planes); good_b.set(planes)
        pageable = [np.array(p) for p in planes]
        ann = HostBuf(fmt, rows, cols); ann.set(planes)
        before = _state(ga, rows, cols, 4)
        for what, sa, sb, c in (("pageable input", pageable, pageable, cols), ("odd cols", good_a.planes, good_b.planes, cols - 1)):
            ra = _push(ga, "host", fmt, sa, n, out_a.planes, cols=c); ea = _err(ctx)
            rb = direct(gb, fmt, sb, n, out_b.planes, c); eb = _err(ctx)
            assert ra[0] == rb[0] == ERR_ARG and ea == eb, (fmt, what, ea, eb)
        # another frame announced: pushing this one first is refused by both with the entry's own message
        for g in (ga, gb):
            g.prefetch_yuv420_host_prepared(g.prepare_yuv420_host(tuple(ann.planes)))
        ra = _push(ga, "host", fmt, good_a.planes, n, out_a.planes); ea = _err(ctx)
        rb = direct(gb, fmt, good_b.planes, n, out_b.planes); eb = _err(ctx)
        assert ra[0] == rb[0] == ERR_ARG and ea == eb and "order announced" in ea, (fmt, ea, eb)
        ctx.sync()
        _assert_state(ga, before, rows, cols, 4, (fmt, "delegate"))
        assert out_a.untouched() and out_b.untouched()
        # the announced frame itself goes through the delegate
        ra = _push(ga, "host", fmt, ann.planes, n, out_a.planes)
        rb = direct(gb, fmt, ann.planes, n, out_b.planes)
        ctx.sync()
        assert ra[:3] == rb == (0, 1, n - DELAY) and np.array_equal(out_a.a, out_b.a) and out_a.guards_intact()
        ga.close(); gb.close()


# ---- restart, then the other format class ---------------------------------------------------------------------------------------------------------
def test_restart_then_the_other_format_class(ctx, oracle):
    n = 9
    clip = _clip(540, 960, 11, 31)
    gd, _ = _filter(ctx, True)
    gh, _ = _filter(ctx, True)
    for fmt, frames in (("BGRA", clip[:n]), ("UYVY", clip[2:2 + n]), ("BGR3", clip[:DELAY + 2])):
        dev = _device_stream(ctx, oracle, gd, frames, [fmt] * len(frames))
        host = _host_stream(ctx, oracle, gh, frames, [fmt] * len(frames), 0, SCHEDULES["mixed"])
        assert sum(h is not None for h in host) == len(frames) - DELAY
        _assert_same(host, dev, ("restart", fmt))
        if fmt == "UYVY":
            _require_live_warp(gh, "after restart")
        gd.restart(); gh.restart()
    gd.close(); gh.close()
