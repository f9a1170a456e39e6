#!/bin/bash
# experiments: one bench line per argument string (extra bench.py arguments)
cd "$(dirname "$0")/../.."; export BENCH_OUT=${BENCH_OUT:-bench_out}; mkdir -p $BENCH_OUT/exp
i=0
for a in "$@"; do
  i=$((i+1))
  timeout 300 python bench.py --full --steps 20 --warmup 3 --cpu-sample 64 --latency-requests 0 $a > $BENCH_OUT/exp/$i.json 2> $BENCH_OUT/exp/$i.log || tail -5 $BENCH_OUT/exp/$i.log
  python - <<PY
import json
d=json.load(open("$BENCH_OUT/exp/$i.json"))
print("$a".ljust(34), round(d['value']/1e6,1),'M items/s', round(d['ms_per_step'],3),'ms', {k:round(v['avg_ms']*v['launches_per_step'],3) for k,v in d['kernels'].items()})
PY
done
