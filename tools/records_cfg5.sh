#!/bin/bash
# tools/records_cfg5.sh : cfg5 at full size (100 M x 768, nlist 65 536, nprobe 512, batch 16 384; streamed GPU encoder) with the
# self-check leg (a --full run, ~10 minutes on the GPU; writes $OUT_DIR/bench_cfg5.json, default bench_records/)
cd "$(dirname "$0")/.."
out=${OUT_DIR:-bench_records}; mkdir -p $out
python bench.py --full --config cfg5 --no-cpu --no-latency --kmeans-iters 3 2> $out/bench_cfg5.err | grep '^{' | tail -n 1 > $out/bench_cfg5.json
python - $out/bench_cfg5.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1])); p = d['pruned']
print('cfg5', round(d['value']), 'q/s', round(d['ms_per_step'], 3), 'ms/step recall', d.get('recall_at_10'), 'roofline', round(d['roofline']['frac'], 3),
      'stream entries/launch', p.get('stream_entries_per_launch'), 'req GB', p['bytes_requested_per_launch'] / 1e9, 'self_check', d.get('self_check'), 'encoder', d.get('encoder'))
PY
