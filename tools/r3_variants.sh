#!/bin/bash
for v in "$@"; do
  export RG_LIB=$PWD/red-gnn_amd/libredgnn_$v.so
  python tools/r3_debug2.py 2>/dev/null | tail -1
  python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-family-eval --no-dense-f32 2>/dev/null | python -c "
import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print('$v', 'ms/step', round(d['ms_per_step'],3), 'dense avg launch ms', round(d['roofline_dense']['avg_launch_ms'],3))"
done
