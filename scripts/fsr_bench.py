"""Times the FSR filter's EASU pass (lvk_hip_fsr_easu through livevisionkit_amd.FSRFilter) with HIP events around back-to-back applies after
a warm-up, and lvk_hip_upscale (the library's own FSR.cl port, ScalingFilter) at 1080p -> 4K as the in-house comparison.

    python scripts/fsr_bench.py [--iters N] [--warmup W]

Cases: 1080p -> 4K in BGRA and BGR, 720p -> 1080p, 4K -> 1080p, and a 1080p centre crop (960 x 540) -> 1080p.  One JSON line per case: mean /
min µs per apply over 5 loops, output pixels, and the kernel path.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`;
VALU instructions: a separate `rocprofv3 --pmc SQ_INSTS_VALU` run."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [  # name, (rows, cols), format, output (rows, cols), crop (l, t, r, b)
    ("1080p_to_4k_bgra", (1080, 1920), 1, (2160, 3840), (0, 0, 0, 0)),
    ("1080p_to_4k_bgr", (1080, 1920), 0, (2160, 3840), (0, 0, 0, 0)),
    ("720p_to_1080p_bgr", (720, 1280), 0, (1080, 1920), (0, 0, 0, 0)),
    ("4k_to_1080p_bgr", (2160, 3840), 0, (1080, 1920), (0, 0, 0, 0)),
    ("1080p_crop_to_1080p_bgr", (1080, 1920), 0, (1080, 1920), (480, 270, 480, 270)),
]


def _time(ctx, stream, fn, iters, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    ctx.sync()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            fn()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1000.0 / iters)
    return float(np.mean(times)), float(min(times))


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
    for name, (rows, cols), fmt, (oh, ow), crop in CASES:
        ch = 4 if fmt == 1 else 3
        f = lvk.FSRFilter(ctx, output_size=(oh, ow), maintain_aspect_ratio=False, crop=crop)
        region, size, skip = f.geometry(rows, cols)
        assert size == (oh, ow) and not skip
        src = torch.from_numpy(rng.integers(0, 256, (rows, cols, ch), dtype=np.uint8)).cuda()
        dst = torch.empty((oh, ow, ch), dtype=torch.uint8, device="cuda")
        us, us_min = _time(ctx, stream, lambda: f.apply(src, fmt, out=dst), a.iters, a.warmup)
        print(json.dumps({"bench": "fsr_easu", "case": name, "rows": rows, "cols": cols, "out_rows": oh, "out_cols": ow, "channels": ch,
                          "path": ["staged", "direct"][ctx.lib.lvk_hip_fsr_easu_path(region[2], region[3], oh, ow)], "iters": a.iters,
                          "us_mean": round(us, 2), "us_min": round(us_min, 2), "out_pixels": oh * ow}), flush=True)
    # the in-house comparison: lvk_hip_upscale (FSR.cl's easu_scale), BGR 1080p -> 4K
    src = torch.from_numpy(rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).cuda()
    dst = torch.empty((2160, 3840, 3), dtype=torch.uint8, device="cuda")

    def upscale():
        rc = ctx.lib.lvk_hip_upscale(ctx.handle, ctypes.c_void_p(src.data_ptr()), 1920 * 3, 1080, 1920, ctypes.c_void_p(dst.data_ptr()), 3840 * 3,
                                     2160, 3840, 0)
        assert rc == 0
    us, us_min = _time(ctx, stream, upscale, a.iters, a.warmup)
    print(json.dumps({"bench": "upscale", "case": "1080p_to_4k_bgr", "iters": a.iters, "us_mean": round(us, 2), "us_min": round(us_min, 2),
                      "out_pixels": 2160 * 3840}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
