"""Times the deblocking filter on the planes of an OBS video format in one call (lvk_hip_deblock_apply_obs) against the three-call chain it replaces
(lvk_hip_ingest_obs -> lvk_hip_deblock_apply -> lvk_hip_egress_obs) for UYVY, I422, I444, AYUV and BGR3 at 1080p and 4K, default settings.

    python scripts/deblock_obs_bench.py [--iters N] [--warmup W] [--loops L] [--size ROWSxCOLS] [--format NAME] [--out FILE]

One process, one build, the GPU otherwise idle.  Both routes read the same input planes (built from the compressed-looking texture of
tests/deblock_px_cases.py, its chroma decimated to the format's sampling) and write output planes of their own; the chain also writes its packed 8UC3
frame, allocated once.  Each route has its own filter object.  The chain is the parent's code, unchanged: it is the yardstick.  The outputs of the two
routes are compared for equality first.  HIP events around a loop of N back-to-back calls, L loops per route after W warm-up calls each, the routes
ALTERNATING loop by loop (a neighbour's load on the host hits both alike); the time of a route is the median of its loops, the spread their minimum and
maximum.  One JSON line per size and format; --out also appends them to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(1080, 1920), (2160, 3840)]
FORMATS = ["UYVY", "I422", "I444", "AYUV", "BGR3"]


def planes_of(fmt, tex):
    """numpy planes of `fmt` from a packed [rows, cols, 3] texture: every second chroma column for 4:2:2 (BGR3: the frame itself)."""
    import numpy as np
    y, u, v = tex[..., 0], tex[..., 1], tex[..., 2]
    if fmt == "I422":
        return [y, u[:, ::2], v[:, ::2]]
    if fmt == "UYVY":
        return [np.ascontiguousarray(np.stack([np.stack([u[:, ::2], v[:, ::2]], axis=2).reshape(y.shape), y], axis=2))]
    if fmt == "I444":
        return [y, u, v]
    if fmt == "AYUV":
        return [np.ascontiguousarray(np.stack([np.full_like(y, 255), y, u, v], axis=2))]
    if fmt == "BGR3":
        return [tex]
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
    from tests.deblock_px_cases import blocky
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    lines = []

    def run(size, fmt):
        rows, cols = size
        frame_format = 0 if fmt == "BGR3" else 4                                 # LVK_FORMAT_BGR / LVK_FORMAT_YUV
        planes = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes_of(fmt, blocky(rows, cols, seed=rows * 7 + cols + 3))]
        out_one = [torch.zeros_like(p) for p in planes]
        out_chain = [torch.zeros_like(p) for p in planes]
        packed = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
        f_one, f_chain = lvk.DeblockingFilter(ctx), lvk.DeblockingFilter(ctx)

        def one():
            f_one.apply_obs(fmt, planes, out=out_one)

        def chain():
            ctx.ingest_obs(fmt, planes, out=packed)
            f_chain.apply(packed, frame_format)
            ctx.egress_obs(fmt, packed, out_chain)

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
        res = {"bench": "deblock_obs", "size": "%dx%d" % size, "format": fmt, "iters": a.iters, "loops": a.loops, "outputs_equal": same}
        for k, t in times.items():
            res[k + "_us_median"] = round(float(np.median(t)), 2); res[k + "_us_min"] = round(min(t), 2); res[k + "_us_max"] = round(max(t), 2)
        res["one_call_over_chain"] = round(res["one_call_us_median"] / res["chain_us_median"], 3)
        s = json.dumps(res)
        print(s, flush=True)
        lines.append(s)
        ctx.sync()
        f_one.close(); f_chain.close()

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
