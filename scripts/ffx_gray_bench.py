"""Times the CAS filter and the FSR filter's EASU pass on one-channel frames against their three-channel kernels.

    python scripts/ffx_gray_bench.py [--iters N] [--warmup W] [--loops L] [--out FILE]

One process, one build, the GPU otherwise idle.  The yardstick of lvk_hip_cas_gray and lvk_hip_fsr_easu_gray is the three-channel kernel of the same
build on the same frame size (lvk_hip_cas, lvk_hip_fsr_easu on a BGR frame): nothing older exists for one-channel frames.  HIP events around a loop of N
launches, L loops per variant after W warm-up launches each, the variants ALTERNATING loop by loop (a neighbour's load on the host hits all alike); the time
of a variant is the median of its loops.  The outputs are compared first: the GRAY result must equal channel 0 of what the three-channel kernel makes of
(g, g, g).  Sizes: CAS at 1080p and 4K; EASU 1080p -> 4K and 4K -> 1080p (staged with one channel, direct with three: the path is reported).
Per pixel the kernels move 1 + 1 against 3 + 3 bytes and GRAY carries a third of the per-channel arithmetic: the achieved bytes per second are reported
next to the times.  One JSON line per result; --out also appends them to a file."""
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
    from livevisionkit_amd.stabilization import FORMAT_BGR
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
        """the same textured plane as a one-channel frame g and as the three-channel frame (g, g, g)"""
        g = np.ascontiguousarray(synth.textured_frame(rows, cols, seed=31)[..., 0])
        return torch.from_numpy(np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))).cuda(), torch.from_numpy(g).cuda()

    def run(name, rows, cols, out_rows, out_cols, variants, outs, extra):
        for fn in variants.values():
            fn()
        ctx.sync()
        same = bool(torch.equal(outs["gray"], outs["three"][..., 0]))
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        ctx.sync()
        times = {k: [] for k in variants}
        for _ in range(a.loops):
            for k, fn in variants.items():
                times[k].append(loop(fn))
        res = {"bench": "ffx_gray", "kernel": name, "rows": rows, "cols": cols, "out_rows": out_rows, "out_cols": out_cols, "iters": a.iters,
               "loops": a.loops, "gray_equals_three_channel_0": same, **extra}
        for k, t in times.items():
            med = float(np.median(t))
            res[k + "_us_median"] = round(med, 2); res[k + "_us_min"] = round(min(t), 2); res[k + "_us_max"] = round(max(t), 2)
            res[k + "_GBps"] = round((3 if k == "three" else 1) * (rows * cols + out_rows * out_cols) / med / 1e3, 1)
        res["gray_over_three"] = round(res["gray_us_median"] / res["three_us_median"], 3)
        emit(res)

    cas, fsr = lvk.CASFilter(ctx, 0.8), lvk.FSRFilter(ctx)
    for rows, cols in ((1080, 1920), (2160, 3840)):
        s3, s1 = frames(rows, cols)
        outs = {"three": torch.empty_like(s3), "gray": torch.empty_like(s1)}
        run("cas", rows, cols, rows, cols, {"three": lambda: cas.apply(s3, FORMAT_BGR, out=outs["three"]), "gray": lambda: cas.apply(s1, out=outs["gray"])},
            outs, {"sharpness": 0.8})
    for (rows, cols), (oh, ow) in (((1080, 1920), (2160, 3840)), ((2160, 3840), (1080, 1920))):
        s3, s1 = frames(rows, cols)
        fsr.configure(output_size=(oh, ow))
        outs = {"three": torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda"), "gray": torch.empty((oh, ow), dtype=torch.uint8, device="cuda")}
        names = ["staged", "direct"]
        run("fsr_easu", rows, cols, oh, ow, {"three": lambda: fsr.apply(s3, FORMAT_BGR, out=outs["three"]), "gray": lambda: fsr.apply(s1, out=outs["gray"])},
            outs, {"three_path": names[ctx.lib.lvk_hip_fsr_easu_path(cols, rows, oh, ow)], "gray_path": names[ctx.lib.lvk_hip_fsr_easu_gray_path(cols, rows, oh, ow)]})
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
