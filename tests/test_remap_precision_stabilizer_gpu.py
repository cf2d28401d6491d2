"""lvk_hip_stab_set_remap_precision on live streams: a 24-frame clip at 480 x 270 through the stabilization filter, both OBS presets, overlap on and off, packed and
I420 frames.  The oracle's stabilizer gives the EXACT frames; a filter in 1LSB mode must track exactly as an EXACT one does (the tracker never sees the remap)
and emit planes within 1 of the oracle's, at most 1e-4 of the stream's bytes different; a mid-stream switch takes effect on the next emitted frame and drops,
repeats or restarts nothing.  GRAY streams accept the setting and stay exact.  require_live_warp: the compared frames carry the tracker's warp."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import clipgen, oracle_lib
from tests.facade import build_facade

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, N, DELAY = 270, 480, 24, 3
MAX_SHARE = 1e-4


def _settings(preset):
    # relaxed quality assurance: the trust factor leaves zero within the clip (the vector-field preset's local mesh keeps few inliers at this size: QA at zero)
    qa = {"min_scene_quality": 0.3, "min_tracking_quality": 0.2} if preset == "homography" else {"min_scene_quality": 0.0, "min_tracking_quality": 0.0}
    return oracle_lib.preset(preset, predictive_samples=DELAY, **qa)


def _filter(ctx, s, overlap, precision=None):
    import livevisionkit_amd as lvk
    g = lvk.StabilizationFilterSettings()
    ctypes.memmove(ctypes.byref(g), ctypes.byref(s), ctypes.sizeof(s))
    f = lvk.StabilizationFilter(g, context=ctx)
    f.set_overlap(overlap)
    assert f.remap_precision == 0, "a stabilizer is created EXACT"
    if precision is not None:
        f.set_remap_precision(precision)
    return f


@pytest.fixture(scope="module")
def streams(oracle):
    """per preset: the packed frames (what FrameIngest makes of the clip's I420 planes, so that the packed and the I420 entry see one stream), their planes,
    and the oracle's frame per timestamp, packed and as I420 planes"""
    clip = clipgen.Clip(ROWS, COLS, N, device="cuda")
    planes = [oracle.egress_yuv420(clip.render444(i).cpu().numpy()) for i in range(N)]
    packed = [oracle.ingest_yuv420(*p) for p in planes]
    out = {"planes": planes, "packed": packed}
    for preset in ("homography", "field"):
        s = _settings(preset)
        ost = oracle_lib.OracleStabilizer(oracle, s)
        want = {}
        for i, f in enumerate(packed):
            w, ts = ost.push(f, ts=i)
            if w is not None:
                want[ts] = (w.copy(), oracle.egress_yuv420(w))
        assert sorted(want) == list(range(N - DELAY))
        oracle_lib.require_live_warp(ost, f"precision stream {preset}")
        ost.close()
        out[preset] = {"settings": s, "want": want}
    return out


def _push(ctx, gst, streams, entry, i):
    """one push through the packed or the I420 entry -> ([planes as numpy] or None, timestamp)"""
    import torch
    if entry == "packed":
        out, ts = gst.apply(torch.from_numpy(streams["packed"][i]).cuda(), timestamp=i)
        outs = None if out is None else [out]
    else:
        outs, ts = gst.apply_yuv420(tuple(torch.from_numpy(p).cuda() for p in streams["planes"][i]), timestamp=i)
    return outs, ts


def _taps(gst):
    return bytes(gst.stats()), [m.tobytes() for m in gst.meshes()], gst.features().tobytes()


def _want(streams, preset, entry, ts):
    w = streams[preset]["want"][ts]
    return [w[0]] if entry == "packed" else list(w[1])


@pytest.mark.parametrize("entry", ["packed", "i420"])
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("preset", ["homography", "field"])
def test_one_lsb_stream_tracks_as_exact_and_stays_within_one(ctx, streams, preset, overlap, entry):
    s = streams[preset]["settings"]
    exact, onelsb = _filter(ctx, s, overlap), _filter(ctx, s, overlap, "1lsb")
    assert onelsb.remap_precision == 1 and ctx.remap_precision == 0, "the stabilizer's setting is its own"
    total = differing = 0
    emitted = []
    for i in range(N):
        (oe, te), (ol, tl) = _push(ctx, exact, streams, entry, i), _push(ctx, onelsb, streams, entry, i)
        ctx.sync()
        assert _taps(exact) == _taps(onelsb), f"frame {i}: stats, meshes or features differ between the modes"
        assert te == tl and (oe is None) == (ol is None) == (i < DELAY)
        if ol is None:
            continue
        emitted.append(tl)
        for k, (e, l, w) in enumerate(zip(oe, ol, _want(streams, preset, entry, tl))):
            assert np.array_equal(e.cpu().numpy(), w), f"EXACT frame {tl} plane {k} differs from the oracle"
            d = np.abs(l.cpu().numpy().astype(np.int16) - w.astype(np.int16))
            assert d.max() <= 1, f"1LSB frame {tl} plane {k}: max |diff| {int(d.max())}"
            total += d.size; differing += int((d != 0).sum())
    assert emitted == list(range(N - DELAY))
    print(f"{preset} overlap={overlap} {entry}: {differing} of {total} bytes differ ({differing / total:.2e})")
    assert differing <= MAX_SHARE * total, f"{differing} of {total} bytes differ"
    assert exact.stats().trust > 0.1
    exact.close(); onelsb.close()


@pytest.mark.parametrize("entry", ["packed", "i420"])
@pytest.mark.parametrize("overlap", [False, True])
def test_switching_mid_stream_takes_effect_on_the_next_emitted_frame(ctx, streams, overlap, entry):
    """EXACT -> 1LSB before push 9 -> EXACT before push 17: every push from DELAY on emits the frame DELAY pushes back (nothing dropped, repeated or restarted),
    the frames emitted in EXACT are the oracle's bytes, those emitted in 1LSB are within 1 -- and the tracker's state is that of a filter never switched."""
    from livevisionkit_amd.context import LvkHipError
    s = streams["homography"]["settings"]
    gst, twin = _filter(ctx, s, overlap), _filter(ctx, s, overlap)
    differing = 0
    for i in range(N):
        if i == 9:
            gst.set_remap_precision("1lsb")
        if i == 17:
            with pytest.raises(LvkHipError):
                gst.set_remap_precision(7)                       # refused: still 1LSB
            assert gst.remap_precision == 1
            gst.set_remap_precision("exact")
        outs, ts = _push(ctx, gst, streams, entry, i)
        _push(ctx, twin, streams, entry, i)
        ctx.sync()
        assert _taps(gst) == _taps(twin), i
        assert (outs is None) == (i < DELAY)
        if outs is None:
            continue
        assert ts == i - DELAY
        for k, (g, w) in enumerate(zip(outs, _want(streams, "homography", entry, ts))):
            d = np.abs(g.cpu().numpy().astype(np.int16) - w.astype(np.int16))
            if 9 <= i < 17:
                assert d.max() <= 1, (i, k, int(d.max()))
                differing += int((d != 0).sum())
            else:
                assert not d.any(), f"push {i} (EXACT): frame {ts} plane {k} differs from the oracle in {int((d != 0).sum())} bytes"
    print(f"overlap={overlap} {entry}: {differing} bytes differ in the 1LSB stretch")
    gst.close(); twin.close()


@pytest.mark.parametrize("overlap", [False, True])
def test_gray_stream_accepts_the_setting_and_stays_exact(ctx, streams, overlap):
    import torch
    s = streams["homography"]["settings"]
    exact, onelsb = _filter(ctx, s, overlap), _filter(ctx, s, overlap, "1lsb")
    emitted = 0
    for i in range(DELAY + 5):
        g = torch.from_numpy(np.ascontiguousarray(streams["packed"][i][..., 0])).cuda()
        (oe, te), (ol, tl) = exact.apply(g, timestamp=i), onelsb.apply(g.clone(), timestamp=i)
        ctx.sync()
        assert te == tl and (oe is None) == (ol is None)
        if oe is not None:
            assert torch.equal(oe, ol), i
            emitted += 1
    assert emitted == 5 and onelsb.remap_precision == 1
    exact.close(); onelsb.close()


def test_cpp_facade_setter(tmp_path, streams):
    """lvk::StabilizationFilter::set_remap_precision and hip::Context::set_remap_precision through tests/cpp/remap_precision_facade.cpp: three frames emitted
    in OneLSB mode against the three an Exact filter emits for the same clip, and WarpMesh::apply on a OneLSB context against an Exact one."""
    exe = build_facade(tmp_path, os.path.join(ROOT, "tests", "cpp", "remap_precision_facade.cpp"))
    n = DELAY + 3
    with open(tmp_path / "clip.bin", "wb") as f:
        for p in streams["packed"][:n]:
            f.write(p.tobytes())
    r = subprocess.run([exe, str(ROWS), str(COLS), str(n), str(DELAY), str(tmp_path / "clip.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "precision facade ok" in r.stdout, (r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(2, 4, ROWS, COLS, 3)          # [exact, one-lsb] x [3 stabilized frames, WarpMesh::apply]
    d = np.abs(got[0].astype(np.int16) - got[1].astype(np.int16))
    print(f"facade: max |diff| {int(d.max())}, {int((d != 0).sum())} of {d.size} bytes differ")
    assert d.max() <= 1 and (d != 0).sum() <= MAX_SHARE * d.size
    assert not np.array_equal(got[0, 0], got[0, 1]), "the emitted frames are distinct frames"
