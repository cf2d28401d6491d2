"""Times the lens filter on I420 / NV12 planes in one call (lvk_hip_lens_apply_yuv420) against the three-call chain it replaces
(lvk_hip_ingest_yuv420 -> lvk_hip_remap_map -> lvk_hip_egress_yuv420) at 1080p and 4K, profile 0 of tests/test_lens_gpu.py, test mode off.

    python scripts/lens_420_bench.py [--iters N] [--warmup W] [--loops L] [--size ROWSxCOLS] [--layout i420|nv12] [--out FILE]

One process, one build, the GPU otherwise idle.  Both routes read the same input planes (the `smooth` texture of tests/lens_420_cases.py) and write output
planes of their own; the chain also writes its two packed 8UC3 frames, allocated once, and reads a map of its own (lvk_hip_lens_map_create), the filter
the one it built.  The outputs of the two routes are compared for equality first.  HIP events around a loop of N calls, L loops per route and layout after
W warm-up calls each, the routes ALTERNATING loop by loop (a neighbour's load on the host hits both alike); the time of a route is the median of its loops,
the spread their minimum and maximum.
Per-kernel times: the same script under `rocprofv3 --kernel-trace --stats -- python scripts/lens_420_bench.py --loops 1 --size 2160x3840 --layout i420`.
One JSON line per size and layout; --out also appends them to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(1080, 1920), (2160, 3840)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--size", default=None, help="ROWSxCOLS: that size only (a profiler run per case)")
    ap.add_argument("--layout", default=None, choices=["i420", "nv12"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import livevisionkit_amd as lvk
    from tests.lens_420_cases import SEED, as_nv12, params_of, texture
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    lines = []

    def run(size, nv12):
        rows, cols = size
        host = texture("smooth", rows, cols, SEED)
        planes = tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in (as_nv12(host) if nv12 else host))
        params = params_of(0, rows, cols)
        lens = lvk.LCFilter(params, False, context=ctx)
        dmap, _ = ctx.lens_map(params, rows, cols)

        def out_planes():
            y = torch.empty(size, dtype=torch.uint8, device="cuda")
            c = torch.empty((rows // 2, cols // 2, 2) if nv12 else (rows // 2, cols // 2), dtype=torch.uint8, device="cuda")
            return (y, c) if nv12 else (y, c, torch.empty_like(c))

        out_one, out_chain = out_planes(), out_planes()
        packed = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
        remapped = torch.empty_like(packed)

        def one():
            lens.apply_yuv420(*planes, out=out_one)

        def chain():
            ctx.ingest_yuv420(*planes, out=packed)
            ctx.remap_map(packed, dmap, bg=(0, 0, 0), yuv=True, out=remapped)
            ctx.egress_yuv420(remapped, nv12=nv12, out=out_chain)

        routes = {"one_call": one, "chain": chain}
        for r in routes.values():
            r()
        ctx.sync()
        same = all(bool(torch.equal(x, y)) for x, y in zip(out_one, out_chain))

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
        res = {"bench": "lens_420", "size": "%dx%d" % size, "layout": "nv12" if nv12 else "i420", "iters": a.iters, "loops": a.loops, "outputs_equal": same}
        for k, t in times.items():
            res[k + "_us_median"] = round(float(np.median(t)), 2); res[k + "_us_min"] = round(min(t), 2); res[k + "_us_max"] = round(max(t), 2)
        res["one_call_over_chain"] = round(res["one_call_us_median"] / res["chain_us_median"], 3)
        s = json.dumps(res)
        print(s, flush=True)
        lines.append(s)
        ctx.sync()
        lens.close()

    sizes = [tuple(int(v) for v in a.size.split("x"))] if a.size else SIZES
    for size in sizes:
        for nv12 in ([a.layout == "nv12"] if a.layout else [False, True]):
            run(size, nv12)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
