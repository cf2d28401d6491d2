"""Times the lens filter on the planes of an OBS video format in one call (lvk_hip_lens_apply_obs) against the three-call chain it replaces
(lvk_hip_ingest_obs -> lvk_hip_lens_apply -> lvk_hip_egress_obs) at 1080p and 4K for UYVY, I422, I444 and AYUV, profile 0 of tests/test_lens_gpu.py,
test mode off.

    python scripts/lens_obs_bench.py [--iters N] [--warmup W] [--loops L] [--size ROWSxCOLS] [--format NAME] [--out FILE]

One process, one build, the GPU otherwise idle.  Both routes read the same input planes (built from the `smooth` texture of tests/lens_420_cases.py, its
chroma repeated to the format's sampling) and write output planes of their own; the chain also writes its two packed 8UC3 frames, allocated once, and
runs a filter object of its own with the same profile.  The chain is the parent's code, unchanged: it is the yardstick.  The outputs of the two routes
are compared for equality first.  HIP events around a loop of N back-to-back calls, L loops per route after W warm-up calls each, the routes ALTERNATING
loop by loop (a neighbour's load on the host hits both alike); the time of a route is the median of its loops, the spread their minimum and maximum.
One JSON line per size and format; --out also appends them to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(1080, 1920), (2160, 3840)]
FORMATS = ["UYVY", "I422", "I444", "AYUV"]


def planes_of(fmt, y, u, v):
    """numpy planes of `fmt` from an I420 texture: the chroma repeated to the format's sampling."""
    import numpy as np
    u2, v2 = np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0)                    # 4:2:2: cols / 2 wide, rows high
    if fmt == "I422":
        return [y, u2, v2]
    if fmt == "UYVY":
        return [np.ascontiguousarray(np.stack([np.stack([u2, v2], axis=2).reshape(y.shape), y], axis=2))]
    u4, v4 = np.repeat(u2, 2, axis=1), np.repeat(v2, 2, axis=1)
    if fmt == "I444":
        return [y, u4, v4]
    if fmt == "AYUV":
        return [np.ascontiguousarray(np.stack([np.full_like(y, 255), y, u4, v4], axis=2))]
    raise ValueError(fmt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--size", default=None, help="ROWSxCOLS: that size only")
    ap.add_argument("--format", default=None, choices=FORMATS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import livevisionkit_amd as lvk
    from livevisionkit_amd.stabilization import FORMAT_YUV
    from tests.lens_420_cases import SEED, params_of, texture
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    lines = []

    def run(size, fmt):
        rows, cols = size
        planes = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes_of(fmt, *texture("smooth", rows, cols, SEED))]
        params = params_of(0, rows, cols)
        lens, lens_chain = lvk.LCFilter(params, False, context=ctx), lvk.LCFilter(params, False, context=ctx)
        out_one, out_chain = [torch.zeros_like(p) for p in planes], [torch.zeros_like(p) for p in planes]
        packed = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
        remapped = torch.empty_like(packed)

        def one():
            lens.apply_obs(fmt, planes, out=out_one)

        def chain():
            ctx.ingest_obs(fmt, planes, out=packed)
            lens_chain.apply(packed, FORMAT_YUV, out=remapped)
            ctx.egress_obs(fmt, remapped, out_chain)

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
        res = {"bench": "lens_obs", "size": "%dx%d" % size, "format": fmt, "iters": a.iters, "loops": a.loops, "outputs_equal": same}
        for k, t in times.items():
            res[k + "_us_median"] = round(float(np.median(t)), 2); res[k + "_us_min"] = round(min(t), 2); res[k + "_us_max"] = round(max(t), 2)
        res["one_call_over_chain"] = round(res["one_call_us_median"] / res["chain_us_median"], 3)
        s = json.dumps(res)
        print(s, flush=True)
        lines.append(s)
        ctx.sync()
        lens.close()
        lens_chain.close()

    sizes = [tuple(int(v) for v in a.size.split("x"))] if a.size else SIZES
    for size in sizes:
        for fmt in ([a.format] if a.format else FORMATS):
            run(size, fmt)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
