"""Times ScalingFilter's two kernels for three, one and four bytes per pixel: the 1080p -> 4K EASU upscale and the 4K RCAS sharpen.

    python scripts/scaling_px_bench.py [--iters N] [--warmup W] [--loops L] [--out FILE]

One process, one build, the GPU otherwise idle.  The yardstick of the one- and four-channel kernels (lvk_hip_upscale_gray / _c4, lvk_hip_sharpen_gray / _c4)
is the three-channel kernel of the same build on the same frame size (lvk_hip_upscale with yuv = 0, lvk_hip_sharpen): nothing older exists for these pixel
sizes.  HIP events around a loop of N launches, L loops per variant after W warm-up launches each, the variants ALTERNATING loop by loop (a neighbour's load
on the host hits all alike); the time of a variant is the median of its loops.  The outputs are compared first: the colour bytes of the four-channel result
and the GRAY result must equal what the three-channel kernel makes of the same content.
Per pixel the kernels move 6 / 2 / 8 bytes (read + write; the upscale reads a quarter of what it writes per axis), and GRAY carries a third of the
three-channel arithmetic: the achieved bytes per second are reported next to the times.  One JSON line per result; --out also appends them to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loops", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import livevisionkit_amd as lvk
    from tests import synth
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

    def frames(rows, cols):
        """the same textured content as a three-, one- and four-channel frame: (c0, c1, c2), c0, (c0, c1, c2, a)"""
        f3 = synth.textured_frame(rows, cols, seed=31)
        alpha = synth.textured_frame(rows, cols, seed=23)[..., 1][::-1]
        f4 = np.ascontiguousarray(np.concatenate([f3, alpha[..., None]], -1))
        return (torch.from_numpy(f3).cuda(), torch.from_numpy(np.ascontiguousarray(f3[..., 0])).cuda(), torch.from_numpy(f4).cuda())

    def run(name, rows, cols, variants, outs, bytes_per_px):
        for fn in variants.values():
            fn()
        ctx.sync()
        # GRAY = channel 0 of the three-channel result on (g, c1, c2) (upscale) -- for RCAS the channels are coupled, so only the four-channel colour is compared
        same = {"c4_colour_equals_three": bool(torch.equal(outs["c4"][..., :3], outs["three"]))}
        if name == "upscale":
            same["gray_equals_three_channel_0"] = bool(torch.equal(outs["gray"], outs["three"][..., 0]))
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        ctx.sync()
        times = {k: [] for k in variants}
        for _ in range(a.loops):
            for k, fn in variants.items():
                times[k].append(loop(fn))
        res = {"bench": "scaling_px", "kernel": name, "rows": rows, "cols": cols, "iters": a.iters, "loops": a.loops, **same}
        for k, t in times.items():
            med = float(np.median(t))
            res[k + "_us_median"] = round(med, 2); res[k + "_us_min"] = round(min(t), 2); res[k + "_us_max"] = round(max(t), 2)
            res[k + "_GBps"] = round(bytes_per_px[k] * rows * cols / med / 1e3, 1)
        res["gray_over_three"] = round(res["gray_us_median"] / res["three_us_median"], 3)
        res["c4_over_three"] = round(res["c4_us_median"] / res["three_us_median"], 3)
        emit(res)

    # ---- 1080p -> 4K upscale (bytes per OUTPUT pixel: the write plus a quarter of a source pixel)
    s3, s1, s4 = frames(1080, 1920)
    size, shape = (3840, 2160), (2160, 3840)
    outs = {"three": torch.empty(shape + (3,), dtype=torch.uint8, device="cuda"), "gray": torch.empty(shape, dtype=torch.uint8, device="cuda"),
            "c4": torch.empty(shape + (4,), dtype=torch.uint8, device="cuda")}
    run("upscale", 2160, 3840, {"three": lambda: ctx.upscale(s3, size, yuv=False, out=outs["three"]), "gray": lambda: ctx.upscale_gray(s1, size, out=outs["gray"]),
                                "c4": lambda: ctx.upscale_c4(s4, size, out=outs["c4"])}, outs, {"three": 3 * 1.25, "gray": 1 * 1.25, "c4": 4 * 1.25})
    # ---- 4K sharpen at ScalingFilter's default sharpness (bytes per pixel: one read, one write)
    s3, s1, s4 = frames(2160, 3840)
    outs = {"three": torch.empty_like(s3), "gray": torch.empty_like(s1), "c4": torch.empty_like(s4)}
    run("sharpen", 2160, 3840, {"three": lambda: ctx.sharpen(s3, 0.8, out=outs["three"]), "gray": lambda: ctx.sharpen_gray(s1, 0.8, out=outs["gray"]),
                                "c4": lambda: ctx.sharpen_c4(s4, 0.8, out=outs["c4"])}, outs, {"three": 6, "gray": 2, "c4": 8})
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
