"""Times the one-channel (GRAY) remap kernels against the three-channel ones, and lvk_hip_stab_push_gray against lvk_hip_stab_push, on the same frames.

    python scripts/gray_bench.py [--iters N] [--warmup W] [--frames F] [--out FILE]

Kernels: at 4K and 1080p, the homography kernel and the 16 x 16 mesh kernel, same size, same warp, the GPU otherwise idle; the one-channel frame is channel
0 of the three-channel one.  HIP events around a synchronised loop of N launches, 5 loops per variant, the two variants ALTERNATING loop by loop (a
neighbour's load on the host hits both alike); the outputs are compared first (the GRAY frame must equal channel 0 of the non-YUV three-channel remap of
(g, 128, 128)).  The three-channel kernels are timed with the program the stabilizer runs on a YUV stream (yuv = 1) and with the one the GRAY kernel is
channel 0 of (yuv = 0).
Stream: the generator's 1080p clip (tests/clipgen.py) through StabilizationFilter.apply as packed YUV frames and as GRAY planes, overlap mode, free-running
pushes, frames per second over F pushes after the queue has filled.
One JSON line per result; --out also appends them to a file.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import livevisionkit_amd as lvk
    from tests import clipgen, synth
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def loop(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.iters):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.iters

    for rows, cols in ((2160, 3840), (1080, 1920)):
        g = torch.Generator(device="cuda"); g.manual_seed(rows)
        src3 = torch.randint(0, 256, (rows, cols, 3), dtype=torch.uint8, device="cuda", generator=g)
        src3[..., 1:] = 128
        src1 = src3[..., 0].contiguous()
        dst3, dst1 = torch.empty_like(src3), torch.empty_like(src1)
        rng = np.random.default_rng(rows)
        H = synth.random_homography(rows, cols, rng, strength=0.5)
        mesh = synth.random_mesh(16, 16, rng, amp=0.02)
        cases = {
            "homography": {"gray": lambda: ctx.remap_homography_gray(src1, H, bg=7, out=dst1),
                           "three_yuv": lambda: ctx.remap_homography(src3, H, bg=(7, 8, 9), yuv=True, out=dst3),
                           "three_rgb": lambda: ctx.remap_homography(src3, H, bg=(7, 8, 9), yuv=False, out=dst3)},
            "mesh16": {"gray": lambda: ctx.remap_mesh_gray(src1, mesh, bg=7, out=dst1),
                       "three_yuv": lambda: ctx.remap_mesh(src3, mesh, bg=(7, 8, 9), yuv=True, out=dst3),
                       "three_rgb": lambda: ctx.remap_mesh(src3, mesh, bg=(7, 8, 9), yuv=False, out=dst3)},
        }
        for name, variants in cases.items():
            variants["three_rgb"](); variants["gray"](); ctx.sync()
            same = bool(torch.equal(dst1, dst3[..., 0]))
            for fn in variants.values():
                for _ in range(a.warmup):
                    fn()
            ctx.sync()
            times = {k: [] for k in variants}
            for _ in range(5):
                for k, fn in variants.items():
                    times[k].append(loop(fn))
            res = {"bench": "gray_remap", "kernel": name, "rows": rows, "cols": cols, "iters": a.iters, "gray_equals_channel0": same}
            for k, t in times.items():
                res[k + "_us_mean"] = round(float(np.mean(t)), 2); res[k + "_us_min"] = round(min(t), 2)
            res["gray_over_three_yuv"] = round(res["gray_us_mean"] / res["three_yuv_us_mean"], 3)
            res["gray_over_three_rgb"] = round(res["gray_us_mean"] / res["three_rgb_us_mean"], 3)
            emit(res)

    # ---- stream rate: the same clip as packed YUV frames (lvk_hip_stab_push) and as GRAY planes (lvk_hip_stab_push_gray)
    rows, cols, n = 1080, 1920, 24
    clip = clipgen.Clip(rows, cols, n, device="cuda")
    yuv = [clip.render444(i) for i in range(n)]
    gray = [f[..., 0].contiguous() for f in yuv]
    s = lvk.StabilizationFilterSettings.obs_preset("homography", strict=False, predictive_samples=4, min_scene_quality=0.3, min_tracking_quality=0.2)
    rates = {"push": [], "push_gray": []}
    for rep in range(3):
        for kind, frames in (("push", yuv), ("push_gray", gray)):
            f = lvk.StabilizationFilter(s, context=ctx); f.set_overlap(True)
            outs = [torch.empty_like(frames[0]) for _ in range(3)]
            for i in range(2 * n):                                       # fill the queue, warm up
                f.apply(frames[i % n], timestamp=i, out=outs[i % 3])
            ctx.sync()
            t0 = time.perf_counter()
            for i in range(a.frames):
                f.apply(frames[i % n], timestamp=2 * n + i, out=outs[i % 3])
            ctx.sync()
            rates[kind].append(a.frames / (time.perf_counter() - t0))
            trust = f.stats().trust
            f.close()
    emit({"bench": "gray_stream", "rows": rows, "cols": cols, "frames": a.frames, "overlap": True, "trust_at_end": round(float(trust), 2),
          "push_fps": [round(r, 1) for r in rates["push"]], "push_gray_fps": [round(r, 1) for r in rates["push_gray"]],
          "gray_over_three": round(float(np.mean(rates["push_gray"]) / np.mean(rates["push"])), 3)})
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
