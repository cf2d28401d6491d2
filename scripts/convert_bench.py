"""Times the format conversion (lvk_hip_reformat through livevisionkit_amd.reformat) at 4K and 1080p for BGR -> YUV, YUV -> BGR,
BGR -> RGBA, YUV -> RGBA, BGR -> GRAY and GRAY -> YUV, with HIP events around a synchronised loop.

    python scripts/convert_bench.py [--iters N] [--warmup W]

One JSON line per case and mode, with the bytes a conversion must move (one read of the source, one write of the destination), the
achieved rate and its share of the 8 TB/s HBM peak:
  cold  each call works on the next of enough (source, destination) pairs to exceed the 256 MiB Infinity Cache, so every call reads and
        writes HBM (one 4K pair is at most 66 MB and would otherwise stay cache-resident)
  warm  the same pair replayed: the Infinity Cache serves it, so this is not an HBM figure
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`, in a run of its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0                    # MI355X peak HBM bandwidth, TB/s
COPY_TBS = 6.29                  # measured device copy rate, TB/s (MI355X_MICROARCH.md)
INFINITY_CACHE = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    import livevisionkit_amd as lvk
    from livevisionkit_amd.convert import CHANNELS
    from livevisionkit_amd.stabilization import FORMAT_BGR, FORMAT_RGBA, FORMAT_YUV, FORMAT_GRAY
    ctx = lvk.Context(0)
    stream = torch.cuda.current_stream()
    names = {FORMAT_BGR: "BGR", FORMAT_RGBA: "RGBA", FORMAT_YUV: "YUV", FORMAT_GRAY: "GRAY"}
    cases = [(FORMAT_BGR, FORMAT_YUV), (FORMAT_YUV, FORMAT_BGR), (FORMAT_BGR, FORMAT_RGBA), (FORMAT_YUV, FORMAT_RGBA), (FORMAT_BGR, FORMAT_GRAY),
             (FORMAT_GRAY, FORMAT_YUV)]
    gen = torch.Generator(device="cuda").manual_seed(1)
    for rows, cols in ((2160, 3840), (1080, 1920)):
        for sf, df in cases:
            sc, dc = CHANNELS[sf], CHANNELS[df]
            floor_bytes = rows * cols * (sc + dc)
            npairs = INFINITY_CACHE // floor_bytes + 2                   # > 256 MiB of distinct buffers
            srcs = [torch.randint(0, 256, (rows, cols, sc), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(npairs)]
            dsts = [torch.empty((rows, cols, dc), dtype=torch.uint8, device="cuda") for _ in range(npairs)]
            for mode in ("cold", "warm"):
                for i in range(a.warmup):
                    k = i % npairs if mode == "cold" else 0
                    lvk.reformat(ctx, srcs[k], sf, df, out=dsts[k])
                ctx.sync()
                times = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for i in range(a.iters):
                        k = i % npairs if mode == "cold" else 0
                        lvk.reformat(ctx, srcs[k], sf, df, out=dsts[k])
                    e1.record(stream)
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1) * 1000.0 / a.iters)
                us = float(np.mean(times))
                tbs = floor_bytes / (us * 1e-6) / 1e12
                print(json.dumps({"bench": "reformat", "case": "%s->%s" % (names[sf], names[df]), "rows": rows, "cols": cols, "mode": mode,
                                  "buffer_pairs": npairs if mode == "cold" else 1, "iters": a.iters, "us_mean": round(us, 2),
                                  "us_min": round(min(times), 2), "floor_bytes": floor_bytes, "tb_per_s": round(tbs, 2),
                                  "hbm_peak_share": round(tbs / HBM_TBS, 3), "copy_rate_share": round(tbs / COPY_TBS, 3)}), flush=True)
            del srcs, dsts
            torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
