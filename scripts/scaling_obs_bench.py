"""Times the scaling filter on the planes of an OBS video format in one call (lvk_hip_scale_obs) against the four-call chain it replaces
(lvk_hip_ingest_obs -> lvk_hip_upscale -> lvk_hip_sharpen -> lvk_hip_egress_obs) for UYVY, I422, I444, AYUV and BGR3 at 540p -> 1080p, 1080p -> 4K and
1080p at equal sizes, sharpness 0.8.

    python scripts/scaling_obs_bench.py [--iters N] [--warmup W] [--loops L] [--size ROWSxCOLS-ROWSxCOLS] [--format NAME] [--out FILE]

One process, one build, the GPU otherwise idle.  Both routes read the same input planes (built from the `smooth` texture of tests/scaling_420_cases.py,
its chroma repeated to the format's sampling) and write output planes of their own; the chain also writes its three packed 8UC3 frames, allocated once.
The chain is the parent's code, unchanged: it is the yardstick.  The outputs of the two routes are compared for equality first.  HIP events around a loop
of N back-to-back calls, L loops per route after W warm-up calls each, the routes ALTERNATING loop by loop (a neighbour's load on the host hits both
alike); the time of a route is the median of its loops, the spread their minimum and maximum.  One JSON line per size pair and format; --out also appends
them to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [((540, 960), (1080, 1920)), ((1080, 1920), (2160, 3840)), ((1080, 1920), (1080, 1920))]
FORMATS = ["UYVY", "I422", "I444", "AYUV", "BGR3"]


def planes_of(fmt, y, u, v):
    """numpy planes of `fmt` from an I420 texture: the chroma repeated to the format's sampling (BGR3: the three full planes as B, G, R)."""
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
    if fmt == "BGR3":
        return [np.ascontiguousarray(np.stack([y, u4, v4], axis=2))]
    raise ValueError(fmt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--size", default=None, help="ROWSxCOLS-ROWSxCOLS: that pair of sizes only")
    ap.add_argument("--format", default=None, choices=FORMATS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import livevisionkit_amd as lvk
    from tests.scaling_420_cases import SEED, texture
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    lines = []

    def run(src, dst, fmt):
        (rows, cols), (drows, dcols) = src, dst
        size = (dcols, drows)
        yuv = fmt != "BGR3"
        planes = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes_of(fmt, *texture("smooth", rows, cols, SEED))]
        shapes = [(p.shape[0] * drows // rows, p.shape[1] * dcols // cols, *p.shape[2:]) for p in planes]
        out_one = [torch.zeros(s, dtype=torch.uint8, device="cuda") for s in shapes]
        out_chain = [torch.zeros(s, dtype=torch.uint8, device="cuda") for s in shapes]
        packed = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
        scaled = torch.empty((drows, dcols, 3), dtype=torch.uint8, device="cuda")
        sharpened = torch.empty_like(scaled)

        def one():
            ctx.scale_obs(fmt, planes, size=size, sharpness=0.8, out=out_one)

        def chain():
            ctx.ingest_obs(fmt, planes, out=packed)
            ctx.upscale(packed, size, yuv=yuv, out=scaled)
            ctx.sharpen(scaled, 0.8, out=sharpened)
            ctx.egress_obs(fmt, sharpened, out_chain)

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
        res = {"bench": "scaling_obs", "src": "%dx%d" % src, "dst": "%dx%d" % dst, "format": fmt, "iters": a.iters, "loops": a.loops, "outputs_equal": same}
        for k, t in times.items():
            res[k + "_us_median"] = round(float(np.median(t)), 2); res[k + "_us_min"] = round(min(t), 2); res[k + "_us_max"] = round(max(t), 2)
        res["one_call_over_chain"] = round(res["one_call_us_median"] / res["chain_us_median"], 3)
        s = json.dumps(res)
        print(s, flush=True)
        lines.append(s)
        ctx.sync()

    if a.size:
        s, d = a.size.split("-")
        pairs = [(tuple(int(v) for v in s.split("x")), tuple(int(v) for v in d.split("x")))]
    else:
        pairs = SIZES
    for src, dst in pairs:
        for fmt in ([a.format] if a.format else FORMATS):
            run(src, dst, fmt)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
