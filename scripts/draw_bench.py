"""Times the device drawing calls (lvk_hip_draw_text / _rect / _points through livevisionkit_amd.draw_*) at 1080p and 4K with HIP events around a
synchronised loop, next to lvk_hip_draw_grid on the same frame as the yardstick.

    python scripts/draw_bench.py [--iters N] [--warmup W]

One JSON line per case: mean / min µs per call over 5 loops.  The HUD is what StabilizationFilter::draw_hud enqueues: the timing text at the
stable region's corner + (5, 40) in blocks of 3, and a rectangle of thickness 2 around the region (the frame less a tenth on each side).
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    import livevisionkit_amd as lvk
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(1)
    colour = (105, 212, 234)
    for rows, cols in ((1080, 1920), (2160, 3840)):
        frame = torch.from_numpy(rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)).cuda()
        region = (cols // 10, rows // 10, cols - 2 * (cols // 10), rows - 2 * (rows // 10))
        origin = (region[0] + 5, region[1] + 40)
        pts = np.c_[rng.uniform(0, cols, 2000), rng.uniform(0, rows, 2000)].astype(np.float32)

        def hud():
            lvk.draw_text(ctx, frame, "0.12ms (3.40ms)", origin, colour, 3, 2)
            lvk.draw_rect(ctx, frame, region, colour, 2)

        cases = (("draw_grid 15 x 15 (yardstick)", lambda: ctx.draw_grid(frame, (15, 15), colour, 1)),
                 ("hud: draw_text + draw_rect", hud),
                 ("draw_text", lambda: lvk.draw_text(ctx, frame, "0.12ms (3.40ms)", origin, colour, 3, 2)),
                 ("draw_rect thickness 2", lambda: lvk.draw_rect(ctx, frame, region, colour, 2)),
                 ("draw_points 2000 x size 10", lambda: lvk.draw_points(ctx, frame, pts, colour, 10)),
                 ("draw_rect filled, full frame", lambda: lvk.draw_rect(ctx, frame, (0, 0, cols, rows), colour, -1)))
        results = {}
        for name, call in cases:
            for _ in range(a.warmup):
                call()
            ctx.sync()
            times = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.iters):
                    call()
                e1.record(stream)
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1000.0 / a.iters)
            results[name] = float(np.mean(times))
            print(json.dumps({"bench": "draw", "case": name, "rows": rows, "cols": cols, "iters": a.iters, "us_mean": round(results[name], 2),
                              "us_min": round(min(times), 2)}), flush=True)
        print(json.dumps({"bench": "draw", "case": "hud / grid", "rows": rows, "cols": cols,
                          "ratio": round(results["hud: draw_text + draw_rect"] / results["draw_grid 15 x 15 (yardstick)"], 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
