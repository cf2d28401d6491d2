"""Times lvk::DeblockingFilter::apply at 4K and 1080p (default settings, YUV frames) with HIP events around a synchronised loop.

    python scripts/deblock_bench.py [--iters N] [--warmup W]

One JSON line per size: mean / min µs per apply over the loop and the HBM-roofline share of the bytes an apply must move (one read of the
frame for statistics + downscale, one read + one write for the blend).  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0        # MI355X peak HBM bandwidth, TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    import livevisionkit_amd as lvk
    from tests.test_deblock_gpu import blocky
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    for rows, cols in ((2160, 3840), (1080, 1920)):
        f = lvk.DeblockingFilter(ctx)
        frame = torch.from_numpy(blocky(rows, cols, seed=1)).cuda()
        for _ in range(a.warmup):
            f.apply(frame, lvk.stabilization.FORMAT_YUV)
        ctx.sync()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.iters):
                f.apply(frame, lvk.stabilization.FORMAT_YUV)
            e1.record(stream)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1000.0 / a.iters)
        x, y, w, h = f.filter_region()
        floor_bytes = 3 * w * h * 3
        us = float(np.mean(times))
        print(json.dumps({"bench": "deblock_apply", "rows": rows, "cols": cols, "region": [w, h], "iters": a.iters, "us_mean": round(us, 2),
                          "us_min": round(min(times), 2), "floor_bytes": floor_bytes,
                          "hbm_roofline_share": round(floor_bytes / (us * 1e-6) / (HBM_TBS * 1e12), 3)}), flush=True)
        f.close()
    ctx.close()


if __name__ == "__main__":
    main()
