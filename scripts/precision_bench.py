"""Times the three-channel remap in its two precisions, LVK_REMAP_EXACT and LVK_REMAP_1LSB, in one process on one build.

    python scripts/precision_bench.py [--iters N] [--warmup W] [--pushes P] [--reps R] [--skip-streams] [--exact-only] [--out FILE]

Kernels: at 4K, the packed homography kernel (lvk_hip_remap_homography), the fused 4:2:0 kernel (lvk_hip_warpmesh_apply_yuv420, 2 x 2 mesh, I420) and the
16 x 16 mesh kernel (lvk_hip_remap_mesh), YUV program, the GPU otherwise idle.  HIP events around a synchronised loop of N launches, 5 loops per mode, the two
modes ALTERNATING loop by loop (a neighbour's load on the host hits both alike); the outputs are compared first (max |diff|, share of differing bytes).
Streams: the workload of `bench.py --streams-per-gpu 4` -- four filters on four HIP stream pairs and four host threads, 4K I420 planes resident in HBM, the
OBS "Homography" preset, overlap on -- driven through the Python mirror with bench.py's own rig; P free-running pushes per stream, R repetitions per mode,
the modes alternating on the SAME filters (lvk_hip_stab_set_remap_precision restarts nothing).
--exact-only: EXACT alone, for a library that predates the mode (LVK_HIP_LIB=<that library>): the plumbing of the mode must cost the default path nothing,
so its figures and this build's EXACT figures should agree within the run-to-run spread.
One JSON line per result; --out also appends them to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pushes", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-streams", action="store_true")
    ap.add_argument("--exact-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from livevisionkit_amd import _native
    if a.exact_only:                      # a library from before the mode does not export its four symbols
        for name in [n for n in _native._SIG if n.endswith("_remap_precision")]:
            del _native._SIG[name]
    import livevisionkit_amd as lvk
    from tests import synth
    modes = ["exact"] if a.exact_only else ["exact", "1lsb"]
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    lines = []

    def emit(d):
        d["library"] = os.path.basename(_native.LIB_PATH)
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def set_mode(obj, mode):
        if not a.exact_only:
            obj.set_remap_precision(mode)

    def loop(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.iters):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.iters

    rows, cols = 2160, 3840
    g = torch.Generator(device="cuda"); g.manual_seed(rows)
    src = torch.randint(0, 256, (rows, cols, 3), dtype=torch.uint8, device="cuda", generator=g)
    dst = torch.empty_like(src)
    rng = np.random.default_rng(rows)
    H = synth.random_homography(rows, cols, rng, strength=0.5)
    mesh2, mesh16 = synth.random_mesh(2, 2, rng, amp=0.02), synth.random_mesh(16, 16, rng, amp=0.02)
    kernels = {"homography": lambda: [ctx.remap_homography(src, H, bg=(7, 8, 9), yuv=True, out=dst)],
               "homography_420": lambda: list(ctx.warpmesh_apply_yuv420(src, mesh2, bg=(7, 8, 9))),
               "mesh16": lambda: [ctx.remap_mesh(src, mesh16, bg=(7, 8, 9), yuv=True, out=dst)]}
    for name, fn in kernels.items():
        outs = {}
        for m in modes:
            set_mode(ctx, m)
            outs[m] = [o.clone() for o in fn()]
            for _ in range(a.warmup):
                fn()
            ctx.sync()
        times = {m: [] for m in modes}
        for _ in range(5):
            for m in modes:
                set_mode(ctx, m)
                times[m].append(loop(fn))
        set_mode(ctx, "exact")
        res = {"bench": "remap_precision_kernel", "kernel": name, "rows": rows, "cols": cols, "iters": a.iters}
        for m in modes:
            res[m + "_us_mean"] = round(float(np.mean(times[m])), 2); res[m + "_us_min"] = round(min(times[m]), 2)
        if len(modes) == 2:
            d = torch.cat([(x.to(torch.int16) - y.to(torch.int16)).abs().flatten() for x, y in zip(outs["exact"], outs["1lsb"])])
            res["max_abs_diff"] = int(d.max()); res["differing_share"] = float((d != 0).float().mean())
            res["1lsb_over_exact"] = round(res["1lsb_us_mean"] / res["exact_us_mean"], 4)
        emit(res)
    del src, dst

    if not a.skip_streams:
        import bench
        K = 4
        device = torch.device("cuda", 0)
        rigs = [bench.Rig(lvk, 0, device, 0x4C564B31 + k, rows, cols, "homography", "i420", "off", True, 48, cut=False, pingpong=True) for k in range(K)]
        try:
            for r in rigs:
                for _ in range(r.delay + 2):
                    r.step()
            bench.run_region(rigs, 100, lambda: None, 0)
            for r in rigs:
                r.sync()
            rates = {m: [] for m in modes}
            for _ in range(a.reps):
                for m in modes:
                    for r in rigs:
                        set_mode(r.filt, m)
                    bench.run_region(rigs, 50, lambda: [r.sync() for r in rigs], 0)
                    dt, em, _ = bench.run_region(rigs, a.pushes, lambda: [r.sync() for r in rigs], 0)
                    rates[m].append(em / dt)
            res = {"bench": "remap_precision_streams", "streams": K, "rows": rows, "cols": cols, "preset": "homography", "format": "i420", "overlap": True,
                   "pushes_per_stream": a.pushes, "trust": [round(float(r.filt.stats().trust), 2) for r in rigs]}
            for m in modes:
                res[m + "_fps"] = [round(x, 1) for x in rates[m]]
            if len(modes) == 2:
                res["1lsb_over_exact"] = round(float(np.mean(rates["1lsb"]) / np.mean(rates["exact"])), 4)
            emit(res)
        finally:
            for r in rigs:
                r.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
