"""Times the FSR filter on the planes of an OBS video format in one call (lvk_hip_fsr_obs) against the three-call chain it replaces
(lvk_hip_ingest_obs -> lvk_hip_fsr_easu -> lvk_hip_egress_obs): 1080p -> 4K and 720p -> 1080p on I420, NV12, UYVY, I444 and AYUV (the staged route: one
launch, planes to planes), and 4K -> 1080p on I420 and UYVY (the direct route: the ingest into a pooled frame, then one launch).

    python scripts/fsr_obs_bench.py [--iters N] [--warmup W] [--loops L] [--scale SRCROWSxSRCCOLS:DSTROWSxDSTCOLS] [--format NAME] [--out FILE]

One process, one build, the GPU otherwise idle.  Both routes read the same input planes (seeded uniform noise, its chroma decimated to the format's
sampling) and write output planes of their own; the chain also writes its two packed 8UC3 frames -- one at the source, one at the output size --,
allocated once.  The chain is the parent's code, unchanged: it is the yardstick.  The outputs of the two routes are compared for equality first.  HIP
events around a loop of N back-to-back calls, L loops per route after W warm-up calls each, the routes ALTERNATING loop by loop (a neighbour's load on
the host hits both alike); the time of a route is the median of its loops, the spread their minimum and maximum.  One JSON line per scale and format;
--out also appends them to a file.  Reads nothing outside the repository."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORMATS = ["I420", "NV12", "UYVY", "I444", "AYUV"]
# (source, output, formats)
SCALES = [((1080, 1920), (2160, 3840), FORMATS), ((720, 1280), (1080, 1920), FORMATS), ((2160, 3840), (1080, 1920), ["I420", "UYVY"])]
FORMAT_YUV = 4                                             # LVK_FORMAT_YUV: what every format here ingests to


def planes_of(fmt, tex):
    """numpy planes of `fmt` from a packed [rows, cols, 3] texture: every second chroma column for 4:2:2, every second row too for 4:2:0."""
    import numpy as np
    y, u, v = tex[..., 0], tex[..., 1], tex[..., 2]
    if fmt == "I420":
        return [y, u[::2, ::2], v[::2, ::2]]
    if fmt == "NV12":
        return [y, np.stack([u[::2, ::2], v[::2, ::2]], axis=2)]
    if fmt == "UYVY":
        return [np.stack([np.stack([u[:, ::2], v[:, ::2]], axis=2).reshape(y.shape), y], axis=2)]
    if fmt == "I444":
        return [y, u, v]
    if fmt == "AYUV":
        return [np.stack([np.full_like(y, 255), y, u, v], axis=2)]
    raise ValueError(fmt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--scale", default=None, help="SRCROWSxSRCCOLS:DSTROWSxDSTCOLS: that scale only, on every format")
    ap.add_argument("--format", default=None, choices=FORMATS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import livevisionkit_amd as lvk
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    lines = []

    def run(size, dst, fmt):
        rows, cols = size
        tex = np.random.default_rng(rows * 1009 + cols).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        planes = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes_of(fmt, tex)]

        def oshape(p):                                         # plane i of the output is the input's plane i at the new size
            return (p.shape[0] * dst[0] // rows, p.shape[1] * dst[1] // cols, *p.shape[2:])

        out_one = [torch.zeros(oshape(p), dtype=torch.uint8, device="cuda") for p in planes]
        out_chain = [torch.zeros(oshape(p), dtype=torch.uint8, device="cuda") for p in planes]
        packed = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
        scaled = torch.empty((dst[0], dst[1], 3), dtype=torch.uint8, device="cuda")
        f = lvk.FSRFilter(ctx, output_size=dst, maintain_aspect_ratio=False)
        path = "direct" if ctx.lib.lvk_hip_fsr_obs_path(cols, rows, dst[0], dst[1]) else "staged"

        def one():
            f.apply_obs(fmt, planes, out=out_one)

        def chain():
            ctx.ingest_obs(fmt, planes, out=packed)
            f.apply(packed, FORMAT_YUV, out=scaled)
            ctx.egress_obs(fmt, scaled, out_chain)

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
        res = {"bench": "fsr_obs", "src": "%dx%d" % size, "dst": "%dx%d" % dst, "format": fmt, "path": path, "iters": a.iters, "loops": a.loops, "outputs_equal": same}
        for k, t in times.items():
            res[k + "_us_median"] = round(float(np.median(t)), 2); res[k + "_us_min"] = round(min(t), 2); res[k + "_us_max"] = round(max(t), 2)
        res["one_call_over_chain"] = round(res["one_call_us_median"] / res["chain_us_median"], 3)
        s = json.dumps(res)
        print(s, flush=True)
        lines.append(s)
        ctx.sync()

    scales = SCALES
    if a.scale:
        src, dst = (tuple(int(v) for v in s.split("x")) for s in a.scale.split(":"))
        scales = [(src, dst, FORMATS)]
    for src, dst, formats in scales:
        for fmt in formats:
            if a.format in (None, fmt):
                run(src, dst, fmt)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
