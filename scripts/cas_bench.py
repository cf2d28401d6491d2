"""Times the CAS filter (lvk_hip_cas through livevisionkit_amd.CASFilter) at 4K and 1080p BGR and 4K BGRA, sharpness 0.8, with HIP events
around a synchronised loop.

    python scripts/cas_bench.py [--iters N] [--warmup W]

One JSON line per case: mean / min µs per apply over 5 loops and the HBM-roofline share of the bytes an apply must move (one read of the
source, one write of the destination).  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`."""
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
    from livevisionkit_amd.stabilization import FORMAT_BGR, FORMAT_BGRA
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    f = lvk.CASFilter(ctx, sharpness=0.8)
    rng = np.random.default_rng(1)
    for rows, cols, fmt, ch in ((2160, 3840, FORMAT_BGR, 3), (1080, 1920, FORMAT_BGR, 3), (2160, 3840, FORMAT_BGRA, 4)):
        src = torch.from_numpy(rng.integers(0, 256, (rows, cols, ch), dtype=np.uint8)).cuda()
        dst = torch.empty_like(src)
        for _ in range(a.warmup):
            f.apply(src, fmt, out=dst)
        ctx.sync()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.iters):
                f.apply(src, fmt, out=dst)
            e1.record(stream)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1000.0 / a.iters)
        floor_bytes = 2 * rows * cols * ch
        us = float(np.mean(times))
        print(json.dumps({"bench": "cas_apply", "rows": rows, "cols": cols, "channels": ch, "iters": a.iters, "us_mean": round(us, 2),
                          "us_min": round(min(times), 2), "floor_bytes": floor_bytes,
                          "hbm_roofline_share": round(floor_bytes / (us * 1e-6) / (HBM_TBS * 1e12), 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
