#!/usr/bin/env python3
"""Host-resident OBS frames that are not 4:2:0: what lvk_hip_stab_push_obs_host buys over the route a host had before it.

One process, one run, three routes alternating loop by loop on the same frames:
  (a) host     lvk_hip_stab_push_obs_host: pinned planes in, pinned planes out;
  (b) staged   the calls that existed before it: lvk_hip_upload per plane, lvk_hip_sync, lvk_hip_stab_push_obs, lvk_hip_download per plane, lvk_hip_sync;
  (c) i420     lvk_hip_stab_push_yuv420_host on I420 at the same size: the yardstick for bytes moved.
Per loop, after a warm-up: frames/s over N pushes (wall clock around pushes that end in lvk_hip_sync; route (a) and (c) also free running, one
synchronise at the end) and p50 / p99 of the wall-clock time of one synchronised frame.  Prints one JSON line per (format, size, route, loop) and a summary.

    python scripts/obs_host_bench.py [--formats UYVY,I444,BGRA] [--sizes 1080x1920,2160x3840] [--frames 200] [--warmup 30] [--loops 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RING = 8


def planes_of(fmt, y, u, v):
    """planes of `fmt` (torch, on the GPU) from a rendered I420 frame: the chroma samples repeated"""
    import torch
    up = lambda p: p.repeat_interleave(2, 0).repeat_interleave(2, 1).contiguous()
    if fmt == "I420":
        return [y.contiguous(), u.contiguous(), v.contiguous()]
    if fmt == "I444":
        return [y.contiguous(), up(u), up(v)]
    rows, cols = y.shape
    if fmt == "UYVY":
        out = torch.empty((rows, cols, 2), dtype=torch.uint8, device=y.device)
        out[:, :, 1] = y
        out[:, 0::2, 0] = u.repeat_interleave(2, 0)
        out[:, 1::2, 0] = v.repeat_interleave(2, 0)
        return [out]
    if fmt == "BGRA":
        return [torch.stack([up(u), y, up(v), torch.full_like(y, 255)], dim=2).contiguous()]
    raise ValueError(fmt)


def percentile(xs, q):
    return float(np.percentile(np.asarray(xs), q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="UYVY,I444,BGRA")
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--loops", type=int, default=3)
    args = ap.parse_args()
    import torch
    import livevisionkit_amd as lvk
    from tests import clipgen
    ctx = lvk.Context(0)
    lib = ctx.lib
    settings = lvk.StabilizationFilterSettings.obs_preset("homography", strict=False, predictive_samples=4)
    summary = []
    for size in args.sizes.split(","):
        rows, cols = (int(x) for x in size.split("x"))
        clip = clipgen.Clip(rows, cols, RING, device="cuda")
        i420 = [clip.render_i420(i) for i in range(RING)]
        torch.cuda.synchronize()
        for fmt in args.formats.split(","):
            dev_in = [planes_of(fmt, *p) for p in i420]

            def make():
                f = lvk.StabilizationFilter(lvk.StabilizationFilterSettings(), context=ctx); f.configure(settings); f.set_overlap(True)
                return f

            # (a) pinned frames of the format
            fa = make()
            a_in = [fa.host_planes_obs(fmt, rows, cols) for _ in range(RING)]
            for hp, dp in zip(a_in, dev_in):
                for h, d in zip(hp, dp):
                    h[...] = d.cpu().numpy()
            a_out = [fa.host_planes_obs(fmt, rows, cols) for _ in range(2)]
            a_in_p = [fa.prepare_obs_host(fmt, p) for p in a_in]; a_out_p = [fa.prepare_obs_host(fmt, p) for p in a_out]
            frame_bytes = sum(p.nbytes for p in a_in[0])
            # (b) the same pinned frames, staged through device planes by the caller
            fb = make()
            b_dev_in = [torch.empty_like(p) for p in dev_in[0]]; b_dev_out = [torch.empty_like(p) for p in dev_in[0]]
            b_in_p = fb.prepare_obs(fmt, b_dev_in); b_out_p = fb.prepare_obs(fmt, b_dev_out)
            # (c) I420 at the same size
            fc = make()
            c_in = [fc.host_planes(rows, cols) for _ in range(RING)]
            for hp, p in zip(c_in, i420):
                for h, d in zip(hp, p):
                    h[...] = d.cpu().numpy()
            c_out = [fc.host_planes(rows, cols) for _ in range(2)]
            c_in_p = [fc.prepare_yuv420_host(p) for p in c_in]; c_out_p = [fc.prepare_yuv420_host(p) for p in c_out]

            def push_a(i):
                fa.apply_obs_host_prepared(a_in_p[i % RING], i, a_out_p[i % 2])

            def push_b(i):
                for d, h in zip(b_dev_in, a_in[i % RING]):
                    ctx._check(lib.lvk_hip_upload(ctx.handle, d.data_ptr(), h.ctypes.data, h.nbytes))
                ctx._check(lib.lvk_hip_sync(ctx.handle))
                got, _ = fb.apply_obs_prepared(b_in_p, i, b_out_p)
                if got is not None:
                    for d, h in zip(b_dev_out, a_out[i % 2]):
                        ctx._check(lib.lvk_hip_download(ctx.handle, h.ctypes.data, d.data_ptr(), h.nbytes))
                ctx._check(lib.lvk_hip_sync(ctx.handle))

            def push_c(i):
                fc.apply_yuv420_host_prepared(c_in_p[i % RING], i, c_out_p[i % 2])

            routes = [("host", push_a, True), ("staged", push_b, False), ("i420", push_c, True)]
            seq = {name: 0 for name, _, _ in routes}
            for loop in range(args.loops):
                for name, push, can_run_free in routes:                  # alternating: whatever else shares the host hits all three alike
                    i = seq[name]
                    for _ in range(args.warmup):
                        push(i); ctx.sync(); i += 1
                    lat = []
                    t0 = time.perf_counter()
                    for _ in range(args.frames):
                        t = time.perf_counter()
                        push(i); ctx.sync(); i += 1
                        lat.append((time.perf_counter() - t) * 1e3)
                    sync_fps = args.frames / (time.perf_counter() - t0)
                    free_fps = None
                    if can_run_free:
                        for _ in range(args.warmup):
                            push(i); i += 1
                        ctx.sync()
                        t0 = time.perf_counter()
                        for _ in range(args.frames):
                            push(i); i += 1
                        ctx.sync()
                        free_fps = args.frames / (time.perf_counter() - t0)
                    seq[name] = i
                    rec = {"format": "I420" if name == "i420" else fmt, "rows": rows, "cols": cols, "route": name, "loop": loop, "frames": args.frames,
                           "frame_bytes": int(rows * cols * 3 // 2 if name == "i420" else frame_bytes),
                           "sync_fps": round(sync_fps, 1), "p50_ms": round(percentile(lat, 50), 4), "p99_ms": round(percentile(lat, 99), 4),
                           "free_fps": None if free_fps is None else round(free_fps, 1)}
                    print(json.dumps(rec), flush=True)
                    summary.append(rec)
            for f in (fa, fb, fc):
                f.close()
    print("\nformat size route: sync frames/s per loop | p50 ms per loop | p99 ms per loop | free-running frames/s per loop")
    block = args.loops * 3                                      # (the I420 yardstick is measured next to every format: one block per format and size)
    for b in range(0, len(summary), block):
        rows_ = summary[b:b + block]
        for name in ("host", "staged", "i420"):
            rs = [r for r in rows_ if r["route"] == name]
            print(f'{rs[0]["format"]:5s} {rs[0]["rows"]}x{rs[0]["cols"]} {name:7s}: ' + " ".join(f'{r["sync_fps"]:.0f}' for r in rs) + " | " +
                  " ".join(f'{r["p50_ms"]:.3f}' for r in rs) + " | " + " ".join(f'{r["p99_ms"]:.3f}' for r in rs) + " | " +
                  " ".join("-" if r["free_fps"] is None else f'{r["free_fps"]:.0f}' for r in rs))
    ctx.close()


if __name__ == "__main__":
    main()
