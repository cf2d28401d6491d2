"""Times DeblockingFilter's apply for three, one and four bytes per pixel at 3840 x 2160 and 1920 x 1080, default settings.

    python scripts/deblock_px_bench.py [--iters N] [--warmup W] [--loops L] [--out FILE]

One process, one build, the GPU otherwise idle.  The yardstick of the one- and four-channel entries (lvk_hip_deblock_apply_gray / _c4) is the three-channel
apply of the same build in the same run on the same `blocky` texture (tests/deblock_px_cases.py: the colour bytes of the four-channel frame, BGR; GRAY is
its byte 0): nothing older exists for these pixel sizes.  HIP events around a loop of N applies (the four kernels each), L loops per variant after W
warm-up applies each, the variants ALTERNATING loop by loop (a neighbour's load on the host hits all alike); the time of a variant is the median of its
loops.  apply works in place, so every loop starts from a fresh copy of the texture (made ahead of the first event); within a loop the frame converges to
its smoothed form, which changes no loop count of any kernel.  The outputs of one apply are compared first: the colour bytes of the four-channel result must
equal the three-channel result, the GRAY result channel 0 of the three-channel YUV filter on (g, g, g).
Expectation from the bytes alone (6 / 2 / 8 per pixel, read + write): GRAY no slower than three channels, four channels within 4 / 3 of three channels plus
the spread between the loops of the run.  One JSON line per size; --out also appends them to a file."""
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
    from tests.deblock_px_cases import BGRA, GRAY, blocky
    BGR, YUV = 0, 4
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    lines = []

    def run(rows, cols):
        f4 = blocky(rows, cols, seed=rows + cols, channels=4)
        src = {"three": torch.from_numpy(np.ascontiguousarray(f4[..., :3])).cuda(), "gray": torch.from_numpy(np.ascontiguousarray(f4[..., 0])).cuda(),
               "c4": torch.from_numpy(f4).cuda()}
        fmt = {"three": BGR, "gray": GRAY, "c4": BGRA}
        work = {k: v.clone() for k, v in src.items()}
        filt = {k: lvk.DeblockingFilter(ctx) for k in src}        # one handle per variant: its buffers and tables stay those of its pixel size
        for k in src:
            filt[k].apply(work[k], fmt[k])
        ggg = src["gray"][..., None].repeat(1, 1, 3).contiguous()
        ref = lvk.DeblockingFilter(ctx)
        ref.apply(ggg, YUV)
        ctx.sync()
        same = {"c4_colour_equals_three": bool(torch.equal(work["c4"][..., :3], work["three"])),
                "gray_equals_three_channel_0": bool(torch.equal(work["gray"], ggg[..., 0])),
                "changed_fraction": round(float((work["c4"] != src["c4"]).float().mean()), 3)}

        def loop(k):
            work[k].copy_(src[k])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.iters):
                filt[k].apply(work[k], fmt[k])
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1000.0 / a.iters

        for k in src:
            for _ in range(a.warmup):
                filt[k].apply(work[k], fmt[k])
        ctx.sync()
        times = {k: [] for k in src}
        for _ in range(a.loops):
            for k in src:
                times[k].append(loop(k))
        res = {"bench": "deblock_px", "rows": rows, "cols": cols, "iters": a.iters, "loops": a.loops, **same}
        for k, t in times.items():
            res[k + "_us_median"] = round(float(np.median(t)), 2); res[k + "_us_min"] = round(min(t), 2); res[k + "_us_max"] = round(max(t), 2)
        res["gray_over_three"] = round(res["gray_us_median"] / res["three_us_median"], 3)
        res["c4_over_three"] = round(res["c4_us_median"] / res["three_us_median"], 3)
        s = json.dumps(res)
        print(s, flush=True)
        lines.append(s)
        for f in list(filt.values()) + [ref]:
            f.close()

    run(2160, 3840)
    run(1080, 1920)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
