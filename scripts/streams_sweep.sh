#!/bin/bash
# K streams on ONE GPU (bench.py --streams-per-gpu K): aggregate frames/s and per-stream latency, K = 1 .. 8.  Output: $OUT (default bench_out/sweep).
O=${OUT:-bench_out/sweep}; mkdir -p $O
for K in 1 2 3 4 6 8; do
python bench.py --full --streams-per-gpu $K --frames-per-step 1 --steps 1000 --warmup 50 --pool 64 --no-cpu-baseline --no-pcie --no-configs --no-multi-stream --no-reference-kernel --no-lookahead > $O/k$K.json 2> $O/k$K.err
python - <<P
import json
d = json.loads(open('$O/k$K.json').read().strip().splitlines()[-1])
lat = d.get('latency_ms', {})
print('K=$K value %.0f sustained %.0f per-frame us %.1f p50 %.3f p99 %.3f' % (d['value'], d['sustained']['frames_per_s'], 1e6 / d['sustained']['frames_per_s'], lat.get('p50', 0), lat.get('p99', 0)), 'remap us', round(d['roofline']['avg_launch_us'], 1))
P
done | tee $O/summary.txt
