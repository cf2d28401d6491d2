"""Times the scaling filter on I420 / NV12 planes in one call (lvk_hip_scale_yuv420) against the four-call chain it replaces
(lvk_hip_ingest_yuv420 -> lvk_hip_upscale -> lvk_hip_sharpen -> lvk_hip_egress_yuv420) at 1080p -> 4K, 720p -> 1080p, 4K -> 4K and 1080p -> 1080p,
sharpness 0.8.

    python scripts/scaling_420_bench.py [--iters N] [--warmup W] [--loops L] [--size ROWSxCOLS-ROWSxCOLS] [--out FILE]

One process, one build, the GPU otherwise idle.  Both routes read the same input planes (the `smooth` texture of tests/scaling_420_cases.py) and write
output planes of their own; the chain also writes its two packed 8UC3 frames and the sharpened one, allocated once.  The outputs of the two routes are
compared for equality first.  HIP events around a loop of N calls, L loops per route and layout after W warm-up calls each, the routes ALTERNATING loop by
loop (a neighbour's load on the host hits both alike); the time of a route is the median of its loops, the spread their minimum and maximum.  The claim
to check: the one call's median is at or below the chain's at each size.
Per-kernel times: the same script under `rocprofv3 --kernel-trace --stats -- python scripts/scaling_420_bench.py --loops 1 --size 2160x3840-2160x3840`.
One JSON line per size and layout; --out also appends them to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [((1080, 1920), (2160, 3840)), ((720, 1280), (1080, 1920)), ((2160, 3840), (2160, 3840)), ((1080, 1920), (1080, 1920))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--size", default=None, help="ROWSxCOLS-ROWSxCOLS (source-destination): that case only (a profiler run per case)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import livevisionkit_amd as lvk
    from tests.scaling_420_cases import SEED, as_nv12, texture
    SHARPNESS = 0.8
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    lines = []

    def run(src, dst, nv12):
        host = texture("smooth", src[0], src[1], SEED)
        planes = tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in (as_nv12(host) if nv12 else host))
        size = (dst[1], dst[0])

        def out_planes():
            y = torch.empty(dst, dtype=torch.uint8, device="cuda")
            c = torch.empty((dst[0] // 2, dst[1] // 2, 2) if nv12 else (dst[0] // 2, dst[1] // 2), dtype=torch.uint8, device="cuda")
            return (y, c) if nv12 else (y, c, torch.empty_like(c))

        out_one, out_chain = out_planes(), out_planes()
        packed = torch.empty((src[0], src[1], 3), dtype=torch.uint8, device="cuda")
        scaled = torch.empty((dst[0], dst[1], 3), dtype=torch.uint8, device="cuda")
        sharp = torch.empty_like(scaled)

        def one():
            ctx.scale_yuv420(*planes, size=size, sharpness=SHARPNESS, out=out_one)

        def chain():
            ctx.ingest_yuv420(*planes, out=packed)
            ctx.upscale(packed, size, yuv=True, out=scaled)
            ctx.sharpen(scaled, SHARPNESS, out=sharp)
            ctx.egress_yuv420(sharp, nv12=nv12, out=out_chain)

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
        res = {"bench": "scaling_420", "src": "%dx%d" % src, "dst": "%dx%d" % dst, "layout": "nv12" if nv12 else "i420", "iters": a.iters, "loops": a.loops,
               "outputs_equal": same}
        for k, t in times.items():
            res[k + "_us_median"] = round(float(np.median(t)), 2); res[k + "_us_min"] = round(min(t), 2); res[k + "_us_max"] = round(max(t), 2)
        res["one_call_over_chain"] = round(res["one_call_us_median"] / res["chain_us_median"], 3)
        s = json.dumps(res)
        print(s, flush=True)
        lines.append(s)

    if a.size:
        s, d = a.size.split("-")
        sizes = [(tuple(int(v) for v in s.split("x")), tuple(int(v) for v in d.split("x")))]
    else:
        sizes = SIZES
    for src, dst in sizes:
        for nv12 in (False, True):
            run(src, dst, nv12)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
