"""The stabilization filter on one-channel (GRAY) device frames: lvk_hip_stab_push_gray through livevisionkit_amd.StabilizationFilter.apply.

Expected frames.  The oracle has no GRAY entry, and neither of its three-channel formats is the GRAY stream on its own: pushed as YUV, (g, 128, 128) is
TRACKED as the GRAY stream is (the tracking luma is channel 0 = g, tests/test_gray_spec.py) but remapped by the YUV program, whose luma mixes the channels;
pushed as BGR / RGB it is remapped by the right program but tracked on cvtColor's grey of (g, 128, 128), which is not g.  So the oracle stabilizer is
pushed (g, 128, 128) as YUV -- tracker, quality assurance and path smoother are then exactly the GRAY stream's -- and the expected frame is the ORACLE's
non-YUV remap (the definition of the one-channel remap) of the delayed (g, 128, 128) frame under the correction that push applied
(OracleStabilizer.meshes()), channel 0.  Compared by timestamp, bit for bit; require_live_warp: the trust factor has left zero."""
import ctypes

import numpy as np
import pytest

from tests import clipgen, oracle_lib

pytestmark = pytest.mark.gpu

ROWS, COLS, N, DELAY = 270, 480, 12, 3
SMALL = (200, 360)


def _three(g):
    f = np.full(g.shape + (3,), 128, np.uint8)
    f[..., 0] = g
    return f


def _settings():
    # relaxed quality assurance: the trust factor leaves zero within the clip, so the compared frames carry the warp the tracker estimated
    return oracle_lib.preset("homography", predictive_samples=DELAY, min_scene_quality=0.3, min_tracking_quality=0.2)


def _filter(ctx, s, overlap=False):
    import livevisionkit_amd as lvk
    g = lvk.StabilizationFilterSettings()
    ctypes.memmove(ctypes.byref(g), ctypes.byref(s), ctypes.sizeof(s))
    f = lvk.StabilizationFilter(g, context=ctx)
    f.set_overlap(overlap)
    return f


def _oracle_run(oracle, planes, s):
    """{timestamp: expected one-channel frame} and the oracle stabilizer (left open for its stats) for a stream of planes (sizes may change)."""
    ost = oracle_lib.OracleStabilizer(oracle, s)
    bg = tuple(int(s.background[i]) for i in range(3))
    big = np.zeros((max(p.shape[0] for p in planes), max(p.shape[1] for p in planes), 3), np.uint8)
    want = {}
    for i, g in enumerate(planes):
        out, ts = ost.push(_three(g), ts=i, out=big)
        if out is not None:
            want[ts] = oracle.warpmesh_apply(_three(planes[ts]), ost.meshes()[1], bg=bg, yuv=False)[..., 0]
    return want, ost


@pytest.fixture(scope="module")
def stream(oracle):
    clip = clipgen.Clip(ROWS, COLS, N, device="cuda")
    planes = [clip.render444(i)[..., 0].cpu().numpy().copy() for i in range(N)]
    s = _settings()
    want, ost = _oracle_run(oracle, planes, s)
    assert sorted(want) == list(range(N - DELAY))
    trust = oracle_lib.require_live_warp(ost, "GRAY stream")
    stats = ost.stats()
    ost.close()
    return {"planes": planes, "want": want, "settings": s, "trust": trust, "stats": stats}


def _push_all(ctx, gst, planes, sync_each):
    import torch
    got = {}
    dev = [torch.from_numpy(p).cuda() for p in planes]
    for i, d in enumerate(dev):
        out, ts = gst.apply(d, timestamp=i)
        if sync_each:
            ctx.sync()
        if out is not None:
            assert out.dim() == 2 and gst.last_format == 5
            got[ts] = out
    ctx.sync()
    return {ts: o.cpu().numpy() for ts, o in got.items()}


@pytest.mark.parametrize("overlap", [False, True])
def test_every_emitted_gray_frame_matches_the_oracle(ctx, stream, overlap):
    gst = _filter(ctx, stream["settings"], overlap)
    assert gst.next_output(ROWS, COLS, 5) is None
    got = _push_all(ctx, gst, stream["planes"], sync_each=not overlap)
    assert sorted(got) == sorted(stream["want"])
    for ts, w in stream["want"].items():
        assert np.array_equal(got[ts], w), (overlap, ts, int((got[ts] != w).sum()))
    st = gst.stats()
    assert st.trust == stream["stats"].trust > 0.1 and st.n_matched == stream["stats"].n_matched and list(st.homography) == list(stream["stats"].homography)
    assert gst.next_output(ROWS, COLS, 5) == (ROWS, COLS, 5)                     # a queued GRAY frame: one byte per pixel, step = cols
    gst.close()


def test_unstabilized_and_cropped_outputs(ctx, oracle, stream):
    """stabilize_output = false: the delayed frame leaves as it came (crop off) or through the scene crop alone (crop on), as for three channels.  Nothing is
    tracked on this path, so the oracle pushed (g, 128, 128) as BGR -- the non-YUV program -- gives the expected frame in channel 0 directly."""
    import torch
    planes = stream["planes"][:DELAY + 3]
    for crop in (0, 1):
        s = _settings(); s.stabilize_output = 0; s.crop_to_stable_region = crop
        ost = oracle_lib.OracleStabilizer(oracle, s)
        gst = _filter(ctx, s)
        region = gst.stable_region(ROWS, COLS)
        emitted = 0
        for i, p in enumerate(planes):
            want, wts = ost.push(_three(p), ts=i, fmt=0)
            out, ts = gst.apply(torch.from_numpy(p).cuda(), timestamp=i); ctx.sync()
            assert (want is None) == (out is None) and wts == ts
            if want is not None:
                assert np.array_equal(out.cpu().numpy(), want[..., 0]), (crop, ts)
                assert crop or np.array_equal(want[..., 0], planes[ts])
                emitted += 1
        assert emitted >= 2
        assert gst.stable_region(ROWS, COLS) == region and 0 < region[2] < COLS and 0 < region[3] < ROWS      # works on a GRAY queue, format-free
        ost.close(); gst.close()


def test_mid_stream_resize_refuses_a_small_output_then_accepts(ctx, oracle, stream):
    """ABI 6's size rule: after the frame size changes the next `delay` pushes emit frames of the OLD size; an output buffer of the new size is refused before
    anything changes, and the same push with a buffer that holds the delayed frame succeeds, bit-exact."""
    import torch
    from livevisionkit_amd.context import LvkHipError
    k = DELAY + 3
    planes = stream["planes"][:k] + [np.ascontiguousarray(p[:SMALL[0], :SMALL[1]]) for p in stream["planes"][k:]]
    want, ost = _oracle_run(oracle, planes, stream["settings"])
    gst = _filter(ctx, stream["settings"])
    got = {}
    for i, p in enumerate(planes):
        d = torch.from_numpy(p).cuda()
        if i == k:
            assert gst.next_output(*SMALL, 5) == (ROWS, COLS, 5)
            before = (gst.features(), bytes(gst.stats()), gst.next_output(*SMALL, 5))
            small = torch.full(SMALL, 0x5A, dtype=torch.uint8, device="cuda")
            with pytest.raises(LvkHipError, match="DELAYED frame's own size"):
                gst.apply(d, timestamp=i, out=small)
            ctx.sync()
            assert (small == 0x5A).all()
            after = (gst.features(), bytes(gst.stats()), gst.next_output(*SMALL, 5))
            assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
        out, ts = gst.apply(d, timestamp=i, out=torch.zeros((ROWS, COLS), dtype=torch.uint8, device="cuda")); ctx.sync()
        if out is not None:
            got[ts] = out.cpu().numpy()
    assert sorted(got) == sorted(want) and got[k].shape == SMALL and got[k - 1].shape == (ROWS, COLS)
    for ts, w in want.items():
        assert np.array_equal(got[ts], w), ts
    oracle_lib.require_live_warp(ost, "GRAY resize")
    ost.close(); gst.close()


def test_one_format_class_per_stream(ctx, oracle, stream):
    """A queue of three-channel frames refuses a GRAY push and the reverse, nothing changes, the next valid push is bit-exact; restart() recovers."""
    import torch
    from livevisionkit_amd.context import LvkHipError
    planes, s = stream["planes"], stream["settings"]

    def state(f, fmt):
        return f.features(), bytes(f.stats()), f.next_output(ROWS, COLS, fmt)

    # GRAY frames queued: a three-channel push is refused
    gst = _filter(ctx, s)
    got = {}
    for i, p in enumerate(planes):
        if i == DELAY + 2:
            before = state(gst, 5)
            with pytest.raises(LvkHipError, match="do not share a queue"):
                gst.apply(torch.from_numpy(_three(p)).cuda(), timestamp=99)
            after = state(gst, 5)
            assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
        out, ts = gst.apply(torch.from_numpy(p).cuda(), timestamp=i); ctx.sync()
        if out is not None:
            got[ts] = out.cpu().numpy()
    for ts, w in stream["want"].items():
        assert np.array_equal(got[ts], w), ts
    gst.restart()
    out, _ = gst.apply(torch.from_numpy(_three(planes[0])).cuda(), timestamp=0)           # after restart() the other class is taken
    assert out is None
    gst.close()

    # three-channel frames queued: a GRAY push is refused
    ost = oracle_lib.OracleStabilizer(oracle, s)
    gst = _filter(ctx, s)
    for i, p in enumerate(planes[:DELAY + 4]):
        if i == DELAY + 2:
            before = state(gst, 4)
            with pytest.raises(LvkHipError, match="do not share a queue"):
                gst.apply(torch.from_numpy(p).cuda(), timestamp=99)
            after = state(gst, 4)
            assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
        want, _ = ost.push(_three(p), ts=i)
        out, ts = gst.apply(torch.from_numpy(_three(p)).cuda(), timestamp=i); ctx.sync()
        assert (want is None) == (out is None)
        if want is not None:
            assert np.array_equal(out.cpu().numpy(), want), i
    ost.close(); gst.close()


def test_overlays_are_refused_on_a_gray_queue(ctx, stream):
    import torch
    from livevisionkit_amd.context import LvkHipError
    gst = _filter(ctx, stream["settings"])
    d = torch.from_numpy(stream["planes"][0]).cuda(); keep = d.clone()
    gst.apply(d, timestamp=0)
    for draw in (gst.draw_trackers, gst.draw_motion_mesh):
        with pytest.raises(LvkHipError, match="three bytes per pixel"):
            draw()
    ctx.sync()
    assert torch.equal(d, keep)
    gst.close()


# ---- the host entry: lvk_hip_stab_push_gray_host through StabilizationFilter.apply_gray_host (pinned planes, one each way) ------------------------------
def _host_push_all(ctx, gst, planes, sync_each, pitch_extra=0):
    ins = [gst.host_plane_gray(max(p.shape[0] for p in planes), max(p.shape[1] for p in planes), pitch_extra) for _ in range(2)]
    got = {}
    for i, p in enumerate(planes):
        src = ins[i % 2][:p.shape[0], :p.shape[1]]
        src[...] = p
        due = gst.next_output(p.shape[0], p.shape[1], 5)
        out = gst.host_plane_gray(due[0], due[1], pitch_extra) if due else None
        if out is not None:
            out[...] = 0x5A
        o, ts = gst.apply_gray_host(src, timestamp=i, out=out)
        src[...] = 0                                               # the plane is the caller's again when the call returns
        if sync_each:
            ctx.sync()
        if o is not None:
            got[ts] = o
    ctx.sync()
    return {ts: np.array(o) for ts, o in got.items()}


@pytest.mark.parametrize("overlap", [False, True])
def test_host_entry_every_emitted_frame_matches_the_oracle(ctx, stream, overlap):
    gst = _filter(ctx, stream["settings"], overlap)
    got = _host_push_all(ctx, gst, stream["planes"], sync_each=not overlap, pitch_extra=13 if overlap else 0)
    assert sorted(got) == sorted(stream["want"])
    for ts, w in stream["want"].items():
        assert np.array_equal(got[ts], w), (overlap, ts, int((got[ts] != w).sum()))
    st = gst.stats()
    assert st.trust == stream["stats"].trust > 0.1 and st.n_matched == stream["stats"].n_matched
    gst.close()


def test_host_entry_resize_refusals_and_format_class(ctx, oracle, stream):
    """The device entry's rules through the host entry: the ABI-6 size rule (a too-small pinned output refused, then accepted), pageable planes, the
    other format class and the other GRAY entry refused -- each before anything is uploaded or queued -- and every emitted frame bit-exact."""
    import torch
    from livevisionkit_amd.context import LvkHipError
    k = DELAY + 3
    planes = stream["planes"][:k] + [np.ascontiguousarray(p[:SMALL[0], :SMALL[1]]) for p in stream["planes"][k:]]
    want, ost = _oracle_run(oracle, planes, stream["settings"])
    gst = _filter(ctx, stream["settings"])
    src = gst.host_plane_gray(ROWS, COLS)
    got = {}

    def state():
        return gst.features(), bytes(gst.stats()), gst.next_output(*SMALL, 5)

    def unchanged(before):
        after = state()
        assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]

    for i, p in enumerate(planes):
        s_ = src[:p.shape[0], :p.shape[1]] if p.shape == (ROWS, COLS) else gst.host_plane_gray(*p.shape)
        s_[...] = p
        if i == k:
            before = state()
            assert before[2] == (ROWS, COLS, 5)
            small = gst.host_plane_gray(*SMALL); small[...] = 0x5A
            with pytest.raises(LvkHipError, match="DELAYED frame's own size"):
                gst.apply_gray_host(s_, timestamp=i, out=small)
            with pytest.raises(LvkHipError, match="PINNED"):
                gst.apply_gray_host(np.array(p), timestamp=i, out=gst.host_plane_gray(ROWS, COLS))           # a pageable input plane
            with pytest.raises(LvkHipError, match="PINNED"):
                gst.apply_gray_host(s_, timestamp=i, out=np.zeros((ROWS, COLS), np.uint8))                   # a pageable output plane
            with pytest.raises(LvkHipError, match="do not share a queue"):
                gst.apply(torch.from_numpy(_three(p)).cuda(), timestamp=i)                                   # three channels onto the GRAY queue
            with pytest.raises(LvkHipError, match="restart\\(\\) before switching between the two"):
                gst.apply(torch.from_numpy(p).cuda(), timestamp=i)                                           # the device GRAY entry onto the host entry's queue
            ctx.sync()
            assert (small == 0x5A).all()
            unchanged(before)
        out = gst.host_plane_gray(ROWS, COLS)
        o, ts = gst.apply_gray_host(s_, timestamp=i, out=out); ctx.sync()
        if o is not None:
            got[ts] = np.array(o)
    assert sorted(got) == sorted(want) and got[k].shape == SMALL and got[k - 1].shape == (ROWS, COLS)
    for ts, w in want.items():
        assert np.array_equal(got[ts], w), ts
    oracle_lib.require_live_warp(ost, "GRAY host resize")
    ost.close()
    # a queue of three-channel frames refuses the host entry; restart() lets it through
    gst.restart()
    gst.apply(torch.from_numpy(_three(planes[0])).cuda(), timestamp=0)
    src[...] = planes[0]
    with pytest.raises(LvkHipError, match="do not share a queue"):
        gst.apply_gray_host(src, timestamp=1)
    gst.restart()
    assert gst.apply_gray_host(src, timestamp=0) == (None, None)
    gst.close()


def test_gray_push_onto_a_queue_of_pool_frames_changes_nothing(ctx, stream):
    """Frames queued by lvk_hip_stab_push_obs live in the filter's pool: a GRAY push (either entry) is refused before the queue's owner flags are touched, and
    the next push_obs is what it would have been (a twin that never saw the refused pushes)."""
    import torch
    from livevisionkit_amd.context import LvkHipError
    planes = stream["planes"]

    def bgr3(p):
        return [torch.from_numpy(_three(p)).cuda()]

    a, b = _filter(ctx, stream["settings"], True), _filter(ctx, stream["settings"], True)
    for i, p in enumerate(planes[:DELAY + 3]):
        if i == DELAY + 1:
            with pytest.raises(LvkHipError, match="restart"):
                a.apply(torch.from_numpy(p).cuda(), timestamp=99)
            host = a.host_plane_gray(ROWS, COLS); host[...] = p
            with pytest.raises(LvkHipError, match="restart"):
                a.apply_gray_host(host, timestamp=99)
        oa, ta = a.apply_obs("BGR3", bgr3(p), timestamp=i)
        ob, tb = b.apply_obs("BGR3", bgr3(p), timestamp=i)
        ctx.sync()
        assert ta == tb and (oa is None) == (ob is None)
        if oa is not None:
            assert torch.equal(oa[0], ob[0]), i
    assert bytes(a.stats()) == bytes(b.stats())
    a.close(); b.close()
