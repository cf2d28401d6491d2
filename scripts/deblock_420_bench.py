"""Times the deblocking of I420 / NV12 planes in one call (lvk_hip_deblock_apply_yuv420) against the three-call chain it replaces
(lvk_hip_ingest_yuv420 -> lvk_hip_deblock_apply -> lvk_hip_egress_yuv420) at 3840 x 2160 and 1920 x 1080, default settings.

    python scripts/deblock_420_bench.py [--iters N] [--warmup W] [--loops L] [--size ROWSxCOLS] [--out FILE]

One process, one build, the GPU otherwise idle.  Both routes read the same input planes (the egress of a `blocky` texture, tests/deblock_px_cases.py) and
write output planes of their own; the chain also writes its packed 8UC3 frame, allocated once.  The outputs of the two routes are compared for equality
first.  HIP events around a loop of N applies, L loops per route and layout after W warm-up applies each, the routes ALTERNATING loop by loop (a
neighbour's load on the host hits both alike); the time of a route is the median of its loops, the spread their minimum and maximum.  Both routes are
out of place, so every apply of a loop does the same work.  The claim to check: the one call's median is below the chain's at both sizes.
Per-kernel times: the same script under `rocprofv3 --kernel-trace --stats -- python scripts/deblock_420_bench.py --loops 1 --size 2160x3840`.
One JSON line per size and layout; --out also appends them to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--size", default=None, help="ROWSxCOLS: that size only (a profiler run per size)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import livevisionkit_amd as lvk
    from tests.deblock_px_cases import blocky
    YUV = 4
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    lines = []

    def run(rows, cols, nv12):
        packed0 = torch.from_numpy(blocky(rows, cols, seed=rows + cols)).cuda()
        planes = tuple(p.clone() for p in ctx.egress_yuv420(packed0, nv12=nv12))
        out_one = tuple(torch.empty_like(p) for p in planes)
        out_chain = tuple(torch.empty_like(p) for p in planes)
        packed = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
        f_one, f_chain = lvk.DeblockingFilter(ctx), lvk.DeblockingFilter(ctx)

        def one():
            f_one.apply_yuv420(*planes, out=out_one)

        def chain():
            ctx.ingest_yuv420(*planes, out=packed)
            f_chain.apply(packed, YUV)
            ctx.egress_yuv420(packed, nv12=nv12, out=out_chain)

        routes = {"one_call": one, "chain": chain}
        for r in routes.values():
            r()
        ctx.sync()
        same = all(bool(torch.equal(x, y)) for x, y in zip(out_one, out_chain))
        changed = float(np.mean([float((x != y).float().mean()) for x, y in zip(out_one, planes)]))

        def loop(r):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.iters):
                r()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1000.0 / a.iters

        for r in routes.values():
            for _ in range(a.warmup):
                r()
        ctx.sync()
        times = {k: [] for k in routes}
        for _ in range(a.loops):
            for k, r in routes.items():
                times[k].append(loop(r))
        res = {"bench": "deblock_420", "rows": rows, "cols": cols, "layout": "nv12" if nv12 else "i420", "iters": a.iters, "loops": a.loops,
               "outputs_equal": same, "changed_fraction": round(changed, 3)}
        for k, t in times.items():
            res[k + "_us_median"] = round(float(np.median(t)), 2); res[k + "_us_min"] = round(min(t), 2); res[k + "_us_max"] = round(max(t), 2)
        res["one_call_over_chain"] = round(res["one_call_us_median"] / res["chain_us_median"], 3)
        s = json.dumps(res)
        print(s, flush=True)
        lines.append(s)
        f_one.close(); f_chain.close()

    sizes = [tuple(int(v) for v in a.size.split("x"))] if a.size else [(2160, 3840), (1080, 1920)]
    for rows, cols in sizes:
        for nv12 in (False, True):
            run(rows, cols, nv12)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
