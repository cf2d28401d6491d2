"""The stabilization filter on four-channel (BGRA / RGBA) frames: lvk_hip_stab_push_c4 through livevisionkit_amd.StabilizationFilter.apply, and
lvk_hip_stab_push_c4_host through apply_c4_host.

Expected frames.  The oracle stabilizer is pushed the colour bytes as BGR (respectively RGB): it tracks cvtColor(..2GRAY) of them and
remaps them with the non-YUV program, so tracker, quality assurance and path smoother are the four-channel stream's own and bytes 0 .. 2 of every emitted
frame are the oracle's emitted frame of the same timestamp.  Byte 3 is channel 1 of the ORACLE's non-YUV remap of the delayed (c0, a, a) frame, background
(b0, b3, b3), under the correction that push applied (OracleStabilizer.meshes(), as tests/test_gray_stabilizer_gpu.py obtains it).  Compared by timestamp,
bit for bit; require_live_warp: the trust factor has left zero."""
import ctypes

import numpy as np
import pytest

from tests import clipgen, oracle_lib

pytestmark = pytest.mark.gpu

ROWS, COLS, N, DELAY = 270, 480, 12, 3
SMALL = (200, 360)
BGRA, RGBA, BGR, RGB, YUV, GRAY = 1, 3, 0, 2, 4, 5            # LVK_FORMAT_*
THREE = {BGRA: BGR, RGBA: RGB}
ALPHA_BG = 66
DEVICE = "cuda"


def _settings():
    # relaxed quality assurance: the trust factor leaves zero within the clip, so the compared frames carry the warp the tracker estimated
    return oracle_lib.preset("homography", predictive_samples=DELAY, min_scene_quality=0.3, min_tracking_quality=0.2)


def _filter(ctx, s, overlap=False):
    import livevisionkit_amd as lvk
    g = lvk.StabilizationFilterSettings()
    ctypes.memmove(ctypes.byref(g), ctypes.byref(s), ctypes.sizeof(s))
    f = lvk.StabilizationFilter(g, context=ctx)
    f.set_overlap(overlap)
    f.set_background_alpha(ALPHA_BG)
    return f


def _caa(f):
    return np.ascontiguousarray(np.stack([f[..., 0], f[..., 3], f[..., 3]], -1))


def _oracle_run(oracle, frames, s, fmt):
    """{timestamp: expected four-channel frame} and the oracle stabilizer (left open for its stats) for a stream of frames (sizes may change)."""
    ost = oracle_lib.OracleStabilizer(oracle, s)
    bg = tuple(int(s.background[i]) for i in range(3))
    big = np.zeros((max(p.shape[0] for p in frames), max(p.shape[1] for p in frames), 3), np.uint8)
    want = {}
    for i, f in enumerate(frames):
        out, ts = ost.push(np.ascontiguousarray(f[..., :3]), ts=i, fmt=THREE[fmt], out=big)
        if out is not None:
            r, c = frames[ts].shape[:2]
            alpha = oracle.warpmesh_apply(_caa(frames[ts]), ost.meshes()[1], bg=(bg[0], ALPHA_BG, ALPHA_BG), yuv=False)[..., 1]
            want[ts] = np.concatenate([out[:r, :c], alpha[..., None]], -1)
    return want, ost


@pytest.fixture(scope="module")
def stream(oracle):
    """the generator's clip with a moving alpha pattern that is no colour plane; the expected frames of the BGRA and of the RGBA stream"""
    clip = clipgen.Clip(ROWS, COLS, N, device=DEVICE)
    yy, xx = np.mgrid[0:ROWS, 0:COLS]
    frames = []
    for i in range(N):
        alpha = ((xx * 3 + yy * 5 + 17 * i) % 251).astype(np.uint8)
        # (the clip's Y in channel 1, which carries 0.587 of cvtColor's grey either way: the tracker sees the clip's texture; U and V swap weights
        #  between BGR and RGB, so the two formats still track different greys)
        colour = clip.render444(i).cpu().numpy()[..., [1, 0, 2]]
        frames.append(np.ascontiguousarray(np.concatenate([colour, alpha[..., None]], -1)))
    s = _settings()
    res = {"frames": frames, "settings": s, "want": {}, "stats": {}}
    for fmt in (BGRA, RGBA):
        want, ost = _oracle_run(oracle, frames, s, fmt)
        assert sorted(want) == list(range(N - DELAY))
        oracle_lib.require_live_warp(ost, "four-channel stream")
        res["want"][fmt] = want; res["stats"][fmt] = ost.stats()
        ost.close()
    assert not np.array_equal(res["want"][BGRA][N - DELAY - 1], res["want"][RGBA][N - DELAY - 1]), "the two formats track different greys"
    return res


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        d = got != want
        raise AssertionError(f"{what}: {int(d.sum())} bytes differ, per byte {[int(d[..., k].sum()) for k in range(4)]}")


def _push_all(ctx, gst, frames, fmt, sync_each):
    import torch
    got = {}
    dev = [torch.from_numpy(p).cuda() for p in frames]
    for i, d in enumerate(dev):
        out, ts = gst.apply(d, timestamp=i, fmt=fmt)
        if sync_each:
            ctx.sync()
        if out is not None:
            assert out.dim() == 3 and out.shape[2] == 4 and gst.last_format == fmt
            got[ts] = out
    ctx.sync()
    return {ts: o.cpu().numpy() for ts, o in got.items()}


@pytest.mark.parametrize("fmt", [BGRA, RGBA])
@pytest.mark.parametrize("overlap", [False, True])
def test_every_emitted_frame_matches_the_oracle(ctx, stream, overlap, fmt):
    gst = _filter(ctx, stream["settings"], overlap)
    assert gst.next_output(ROWS, COLS, fmt) is None
    got = _push_all(ctx, gst, stream["frames"], fmt, sync_each=not overlap)
    assert sorted(got) == sorted(stream["want"][fmt])
    for ts, w in stream["want"][fmt].items():
        _same(got[ts], w, (overlap, fmt, ts))
    st, ref = gst.stats(), stream["stats"][fmt]
    assert st.trust == ref.trust > 0.1 and st.n_matched == ref.n_matched and list(st.homography) == list(ref.homography)
    assert gst.next_output(ROWS, COLS, fmt) == (ROWS, COLS, fmt)                 # a queued four-channel frame is reported with its own format
    gst.close()


def test_unstabilized_and_cropped_outputs(ctx, oracle, stream):
    """stabilize_output = false: the delayed frame leaves as it came (crop off) or through the scene crop alone (crop on), as for three channels."""
    import torch
    frames = stream["frames"][:DELAY + 3]
    for crop in (0, 1):
        s = _settings(); s.stabilize_output = 0; s.crop_to_stable_region = crop
        ost, osa = oracle_lib.OracleStabilizer(oracle, s), oracle_lib.OracleStabilizer(oracle, s)
        gst = _filter(ctx, s)
        region = gst.stable_region(ROWS, COLS)
        emitted = 0
        for i, f in enumerate(frames):
            want, wts = ost.push(np.ascontiguousarray(f[..., :3]), ts=i, fmt=BGR)
            # nothing is tracked on this path: a second oracle filter pushed (c0, a, a) applies the same crop and gives byte 3 in its channel 1
            wa, _ = osa.push(_caa(f), ts=i, fmt=BGR)
            out, ts = gst.apply(torch.from_numpy(f).cuda(), timestamp=i, fmt=BGRA); ctx.sync()
            assert (want is None) == (out is None) and wts == ts
            if want is not None:
                got = out.cpu().numpy()
                assert np.array_equal(got[..., :3], want), (crop, ts)
                # (the crop's mesh maps no pixel outside the frame: the background, which the two oracle filters share, never shows)
                assert np.array_equal(got[..., 3], wa[..., 1]), (crop, ts)
                assert crop or np.array_equal(got, frames[ts])
                emitted += 1
        assert emitted >= 2
        assert gst.stable_region(ROWS, COLS) == region and 0 < region[2] < COLS and 0 < region[3] < ROWS
        ost.close(); osa.close(); gst.close()


def test_mid_stream_resize_refuses_a_small_output_then_accepts(ctx, oracle, stream):
    """The size rule: after the frame size changes the next `delay` pushes emit frames of the OLD size; an output buffer of the new size is refused before
    anything changes, and the same push with a buffer that holds the delayed frame succeeds, bit-exact."""
    import torch
    from livevisionkit_amd.context import LvkHipError
    k = DELAY + 3
    frames = stream["frames"][:k] + [np.ascontiguousarray(p[:SMALL[0], :SMALL[1]]) for p in stream["frames"][k:]]
    want, ost = _oracle_run(oracle, frames, stream["settings"], BGRA)
    gst = _filter(ctx, stream["settings"])
    got = {}
    for i, p in enumerate(frames):
        d = torch.from_numpy(p).cuda()
        if i == k:
            assert gst.next_output(*SMALL, BGRA) == (ROWS, COLS, BGRA)
            before = (gst.features(), bytes(gst.stats()), gst.next_output(*SMALL, BGRA))
            small = torch.full(SMALL + (4,), 0x5A, dtype=torch.uint8, device="cuda")
            with pytest.raises(LvkHipError, match="DELAYED frame's own size"):
                gst.apply(d, timestamp=i, out=small, fmt=BGRA)
            ctx.sync()
            assert (small == 0x5A).all()
            after = (gst.features(), bytes(gst.stats()), gst.next_output(*SMALL, BGRA))
            assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
        out, ts = gst.apply(d, timestamp=i, out=torch.zeros((ROWS, COLS, 4), dtype=torch.uint8, device="cuda"), fmt=BGRA); ctx.sync()
        if out is not None:
            got[ts] = out.cpu().numpy()
    assert sorted(got) == sorted(want) and got[k].shape == SMALL + (4,) and got[k - 1].shape == (ROWS, COLS, 4)
    for ts, w in want.items():
        _same(got[ts], w, ts)
    oracle_lib.require_live_warp(ost, "four-channel resize")
    ost.close(); gst.close()


def test_one_pixel_size_per_stream(ctx, stream):
    """A queue holds frames of 1, 3 or 4 bytes per pixel, and BGRA or RGBA: a push of another class is refused in every direction, the filter's state is
    what it was, and the stream goes on bit-exact; restart() recovers."""
    import torch
    from livevisionkit_amd.context import LvkHipError
    frames, s = stream["frames"], stream["settings"]
    c4 = [torch.from_numpy(f).cuda() for f in frames]
    c3 = [t[..., :3].contiguous() for t in c4]
    c1 = [t[..., 0].contiguous() for t in c4]
    pushes = {"BGRA": lambda f, i, ts: f.apply(c4[i], timestamp=ts, fmt=BGRA), "RGBA": lambda f, i, ts: f.apply(c4[i], timestamp=ts, fmt=RGBA),
              "BGR": lambda f, i, ts: f.apply(c3[i], timestamp=ts, fmt=BGR), "YUV": lambda f, i, ts: f.apply(c3[i], timestamp=ts, fmt=YUV),
              "GRAY": lambda f, i, ts: f.apply(c1[i], timestamp=ts)}
    query = {"BGRA": BGRA, "RGBA": RGBA, "BGR": BGR, "YUV": YUV, "GRAY": GRAY}
    clashes = [("BGRA", "RGBA"), ("BGRA", "BGR"), ("BGRA", "GRAY"), ("RGBA", "BGRA"), ("RGBA", "YUV"), ("BGR", "BGRA"), ("YUV", "RGBA"), ("GRAY", "BGRA"), ("GRAY", "RGBA")]
    for queued, other in clashes:
        gst, twin = _filter(ctx, s), _filter(ctx, s)                         # the twin never sees the refused push
        for i in range(DELAY + 3):
            if i == DELAY + 1:
                before = (gst.features(), bytes(gst.stats()), gst.next_output(ROWS, COLS, query[queued]))
                with pytest.raises(LvkHipError, match="do not share a queue"):
                    pushes[other](gst, i, 99)
                after = (gst.features(), bytes(gst.stats()), gst.next_output(ROWS, COLS, query[queued]))
                assert np.array_equal(before[0], after[0]) and before[1:] == after[1:], (queued, other)
            a, ta = pushes[queued](gst, i, i); b, tb = pushes[queued](twin, i, i); ctx.sync()
            assert ta == tb and (a is None) == (b is None), (queued, other, i)
            if a is not None:
                assert torch.equal(a, b), (queued, other, i)
                if queued in ("BGRA", "RGBA"):
                    _same(a.cpu().numpy(), stream["want"][query[queued]][ta], (queued, other, ta))
        assert bytes(gst.stats()) == bytes(twin.stats())
        gst.restart()
        out, _ = pushes[other](gst, 0, 0)                                     # after restart() the other class is taken
        assert out is None
        gst.close(); twin.close()


def test_three_channel_entries_keep_refusing_four_channel_formats(ctx, stream):
    import torch
    from livevisionkit_amd.context import LvkHipError
    gst = _filter(ctx, stream["settings"])
    three = torch.from_numpy(np.ascontiguousarray(stream["frames"][0][..., :3])).cuda()
    for fmt in (BGRA, RGBA):
        with pytest.raises(LvkHipError):
            gst.apply(three, timestamp=0, fmt=fmt)                            # a [rows, cols, 3] tensor goes to lvk_hip_stab_push, which refuses the format
    rc = ctx.lib.lvk_hip_stab_push_c4(gst.handle, three.data_ptr(), three.stride(0), ROWS, COLS * 3 // 4, 0, BGR, None, 0, 0, None, None, None, None)
    assert rc == -1                                                           # ... and the four-channel entry takes BGRA / RGBA only
    assert gst.next_output(ROWS, COLS, BGRA) is None
    gst.close()


def test_misaligned_frames_are_refused_before_anything_changes(ctx, stream):
    import torch
    gst = _filter(ctx, stream["settings"])
    buf = torch.zeros((ROWS * (COLS * 4 + 6) + 16,), dtype=torch.uint8, device="cuda")
    p, step = buf.data_ptr(), 4 * COLS
    for ptr, st_ in ((p + 1, step), (p + 2, step), (p, step + 2), (p, step - 4), (None, step)):
        assert ctx.lib.lvk_hip_stab_push_c4(gst.handle, ptr, st_, ROWS, COLS, 0, BGRA, None, 0, 0, None, None, None, None) == -1, (ptr, st_)
    assert gst.next_output(ROWS, COLS, BGRA) is None and len(gst.features()) == 0
    gst.close()


def test_overlays_are_refused_on_a_four_channel_queue(ctx, stream):
    import torch
    from livevisionkit_amd.context import LvkHipError
    gst = _filter(ctx, stream["settings"])
    d = torch.from_numpy(stream["frames"][0]).cuda(); keep = d.clone()
    gst.apply(d, timestamp=0, fmt=BGRA)
    for draw in (gst.draw_trackers, gst.draw_motion_mesh):
        with pytest.raises(LvkHipError, match="three bytes per pixel"):
            draw()
    ctx.sync()
    assert torch.equal(d, keep)
    gst.close()


# ---- the host entry: lvk_hip_stab_push_c4_host through StabilizationFilter.apply_c4_host (pinned planes, one each way) ----------------------------------
def _host_push_all(ctx, gst, frames, fmt, sync_each, pitch_extra=0):
    ins = [gst.host_plane_c4(max(p.shape[0] for p in frames), max(p.shape[1] for p in frames), pitch_extra) for _ in range(2)]
    got = {}
    for i, p in enumerate(frames):
        src = ins[i % 2][:p.shape[0], :p.shape[1]]
        src[...] = p
        due = gst.next_output(p.shape[0], p.shape[1], fmt)
        out = gst.host_plane_c4(due[0], due[1], pitch_extra) if due else None
        if out is not None:
            out[...] = 0x5A
        o, ts = gst.apply_c4_host(src, timestamp=i, out=out, fmt=fmt)
        src[...] = 0                                               # the plane is the caller's again when the call returns
        if sync_each:
            ctx.sync()
        if o is not None:
            assert gst.last_format == fmt
            got[ts] = o
    ctx.sync()
    return {ts: np.array(o) for ts, o in got.items()}


@pytest.mark.parametrize("overlap,fmt,pitch_extra", [(False, BGRA, 0), (True, RGBA, 12), (True, BGRA, 4)])
def test_host_entry_every_emitted_frame_matches_the_oracle(ctx, stream, overlap, fmt, pitch_extra):
    gst = _filter(ctx, stream["settings"], overlap)
    got = _host_push_all(ctx, gst, stream["frames"], fmt, sync_each=not overlap, pitch_extra=pitch_extra)
    assert sorted(got) == sorted(stream["want"][fmt])
    for ts, w in stream["want"][fmt].items():
        _same(got[ts], w, (overlap, fmt, ts))
    st, ref = gst.stats(), stream["stats"][fmt]
    assert st.trust == ref.trust > 0.1 and st.n_matched == ref.n_matched
    gst.close()


def test_host_entry_refusals(ctx, stream):
    """What lvk_hip_stab_push_c4_host refuses before anything is uploaded or queued: a pageable plane either way, an output plane that is too small or
    not dword-addressable, frames of the device entry still queued (and the reverse), another pixel size in the queue, outstanding 4:2:0 look-ahead --
    and the stream goes on bit-exact."""
    import torch
    from livevisionkit_amd.context import LvkHipError
    frames, want = stream["frames"], stream["want"][BGRA]
    gst = _filter(ctx, stream["settings"])
    src = gst.host_plane_c4(ROWS, COLS)
    got = {}

    def state():
        return gst.features(), bytes(gst.stats()), gst.next_output(ROWS, COLS, BGRA)

    for i, p in enumerate(frames):
        src[...] = p
        if i == DELAY + 2:
            before = state()
            small = gst.host_plane_c4(*SMALL); small[...] = 0x5A
            with pytest.raises(LvkHipError, match="DELAYED frame's own size"):
                gst.apply_c4_host(src, timestamp=i, out=small)
            with pytest.raises(LvkHipError, match="PINNED"):
                gst.apply_c4_host(np.array(p), timestamp=i, out=gst.host_plane_c4(ROWS, COLS))                # a pageable input plane
            with pytest.raises(LvkHipError, match="PINNED"):
                gst.apply_c4_host(src, timestamp=i, out=np.zeros((ROWS, COLS, 4), np.uint8))                  # a pageable output plane
            odd = gst.host_plane_c4(ROWS, COLS, pitch_extra=6)
            with pytest.raises(LvkHipError, match="multiple of 4"):
                gst.apply_c4_host(src, timestamp=i, out=odd)                                                   # an output pitch the kernel cannot address
            with pytest.raises(LvkHipError, match="do not share a queue"):
                gst.apply(torch.from_numpy(np.ascontiguousarray(p[..., :3])).cuda(), timestamp=i, fmt=BGR)    # three channels onto the queue
            with pytest.raises(LvkHipError, match="do not share a queue"):
                gst.apply_c4_host(src, timestamp=i, fmt=RGBA)                                                  # RGBA onto the BGRA queue
            with pytest.raises(LvkHipError, match="restart\\(\\) before switching between the two"):
                gst.apply(torch.from_numpy(p).cuda(), timestamp=i, fmt=BGRA)                                   # the device entry onto the host entry's queue
            ctx.sync()
            assert (small == 0x5A).all()
            after = state()
            assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
        o, ts = gst.apply_c4_host(src, timestamp=i, out=gst.host_plane_c4(ROWS, COLS)); ctx.sync()
        if o is not None:
            got[ts] = np.array(o)
    assert sorted(got) == sorted(want)
    for ts, w in want.items():
        _same(got[ts], w, ts)
    # the device entry's frames queued: the host entry is refused; restart() lets it through
    gst.restart()
    gst.apply(torch.from_numpy(frames[0]).cuda(), timestamp=0, fmt=BGRA)
    src[...] = frames[0]
    with pytest.raises(LvkHipError, match="restart\\(\\) before switching between the two"):
        gst.apply_c4_host(src, timestamp=1)
    gst.restart()
    # outstanding 4:2:0 look-ahead: a frame announced through lvk_hip_stab_prefetch_yuv420_host and not pushed yet
    planes = gst.host_planes(ROWS, COLS)
    for pl in planes:
        pl[...] = 128
    gst.prefetch_yuv420_host_prepared(gst.prepare_yuv420_host(planes))
    with pytest.raises(LvkHipError, match="prefetch"):
        gst.apply_c4_host(src, timestamp=0)
    gst.prefetch_cancel()
    assert gst.apply_c4_host(src, timestamp=0) == (None, None)
    gst.close()
