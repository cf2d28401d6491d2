"""Times the four-channel (BGRA / RGBA) remap kernels against the three-channel ones and against the route a caller had before them, and lvk_hip_stab_push_c4
against lvk_hip_stab_push, on the same frames.

    python scripts/c4_bench.py [--iters N] [--warmup W] [--frames F] [--out FILE]

Kernels: at 1080p and 4K, the homography kernel and the 16 x 16 mesh kernel, same size, same warp, the GPU otherwise idle.  Three variants:
  c4          the four-channel kernel on the BGRA frame;
  three_rgb   the three-channel non-YUV kernel on the same colour content (the bare kernel: what one channel more costs);
  three_pass  lvk_hip_reformat BGRA -> BGR, the three-channel non-YUV remap, lvk_hip_reformat BGR -> BGRA (alpha comes back constant).
HIP events around a synchronised loop of N launches, 5 loops per variant, the variants ALTERNATING loop by loop (a neighbour's load on the host hits all
alike); the outputs are compared first: bytes 0 .. 2 of the four-channel output must equal the three-channel remap, and the three-pass route's colour too.
The condition set in advance: c4 beats three_pass at every size ("c4_beats_three_pass").  The ratio to three_rgb is reported, not gated.
Stream: the generator's 1080p clip (tests/clipgen.py) through StabilizationFilter.apply as BGR frames and as BGRA frames, overlap mode, free-running pushes,
frames per second over F pushes after the queue has filled.
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
    from livevisionkit_amd import stabilization as st
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

    bg4, bg3 = (7, 8, 9, 10), (7, 8, 9)
    for rows, cols in ((1080, 1920), (2160, 3840)):
        g = torch.Generator(device="cuda"); g.manual_seed(rows)
        src4 = torch.randint(0, 256, (rows, cols, 4), dtype=torch.uint8, device="cuda", generator=g)
        src3 = src4[..., :3].contiguous()
        dst4, dst3, tmp3, back4 = torch.empty_like(src4), torch.empty_like(src3), torch.empty_like(src3), torch.empty_like(src4)
        rng = np.random.default_rng(rows)
        H = synth.random_homography(rows, cols, rng, strength=0.5)
        mesh = synth.random_mesh(16, 16, rng, amp=0.02)

        def three_pass(remap):
            lvk.reformat(ctx, src4, st.FORMAT_BGRA, st.FORMAT_BGR, out=tmp3)
            remap(tmp3, dst3)
            lvk.reformat(ctx, dst3, st.FORMAT_BGR, st.FORMAT_BGRA, out=back4)

        cases = {
            "homography": {"c4": lambda: ctx.remap_homography_c4(src4, H, bg=bg4, out=dst4),
                           "three_rgb": lambda: ctx.remap_homography(src3, H, bg=bg3, yuv=False, out=dst3),
                           "three_pass": lambda: three_pass(lambda s, d: ctx.remap_homography(s, H, bg=bg3, yuv=False, out=d))},
            "mesh16": {"c4": lambda: ctx.remap_mesh_c4(src4, mesh, bg=bg4, out=dst4),
                       "three_rgb": lambda: ctx.remap_mesh(src3, mesh, bg=bg3, yuv=False, out=dst3),
                       "three_pass": lambda: three_pass(lambda s, d: ctx.remap_mesh(s, mesh, bg=bg3, yuv=False, out=d))},
        }
        for name, variants in cases.items():
            variants["c4"](); variants["three_rgb"](); ctx.sync()
            same = bool(torch.equal(dst4[..., :3], dst3))
            variants["three_pass"](); ctx.sync()
            same = same and bool(torch.equal(back4[..., :3], dst4[..., :3]))
            for fn in variants.values():
                for _ in range(a.warmup):
                    fn()
            ctx.sync()
            times = {k: [] for k in variants}
            for _ in range(5):
                for k, fn in variants.items():
                    times[k].append(loop(fn))
            res = {"bench": "c4_remap", "kernel": name, "rows": rows, "cols": cols, "iters": a.iters, "colour_equals_three_channel": same}
            for k, t in times.items():
                res[k + "_us_mean"] = round(float(np.mean(t)), 2); res[k + "_us_min"] = round(min(t), 2)
            res["c4_over_three_rgb"] = round(res["c4_us_mean"] / res["three_rgb_us_mean"], 3)
            res["c4_over_three_pass"] = round(res["c4_us_mean"] / res["three_pass_us_mean"], 3)
            res["c4_beats_three_pass"] = bool(max(times["c4"]) < min(times["three_pass"]))
            emit(res)

    # ---- stream rate: the same clip as BGR frames (lvk_hip_stab_push) and as BGRA frames (lvk_hip_stab_push_c4)
    rows, cols, n = 1080, 1920, 24
    clip = clipgen.Clip(rows, cols, n, device="cuda")
    bgr = [clip.render444(i)[..., [1, 0, 2]].contiguous() for i in range(n)]           # the clip's texture where cvtColor's grey weighs most
    bgra = [torch.cat([f, torch.full((rows, cols, 1), 200, dtype=torch.uint8, device="cuda")], -1).contiguous() for f in bgr]
    s = lvk.StabilizationFilterSettings.obs_preset("homography", strict=False, predictive_samples=4, min_scene_quality=0.3, min_tracking_quality=0.2)
    rates = {"push": [], "push_c4": []}
    for rep in range(3):
        for kind, frames, fmt in (("push", bgr, st.FORMAT_BGR), ("push_c4", bgra, st.FORMAT_BGRA)):
            f = lvk.StabilizationFilter(s, context=ctx); f.set_overlap(True)
            outs = [torch.empty_like(frames[0]) for _ in range(3)]
            for i in range(2 * n):                                       # fill the queue, warm up
                f.apply(frames[i % n], timestamp=i, out=outs[i % 3], fmt=fmt)
            ctx.sync()
            t0 = time.perf_counter()
            for i in range(a.frames):
                f.apply(frames[i % n], timestamp=2 * n + i, out=outs[i % 3], fmt=fmt)
            ctx.sync()
            rates[kind].append(a.frames / (time.perf_counter() - t0))
            trust = f.stats().trust
            f.close()
    emit({"bench": "c4_stream", "rows": rows, "cols": cols, "frames": a.frames, "overlap": True, "trust_at_end": round(float(trust), 2),
          "push_fps": [round(r, 1) for r in rates["push"]], "push_c4_fps": [round(r, 1) for r in rates["push_c4"]],
          "c4_over_three": round(float(np.mean(rates["push_c4"]) / np.mean(rates["push"])), 3)})
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
