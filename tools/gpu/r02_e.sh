# round 2, fifth GPU pass: grouped prefetch (c2 / c3 / c4x), BASELINE config #2 as written (XGBoost 100 x depth 6) and
# Metarank's XGBoost default depth 8 on the tree-walk scorer, phase clocks of the c2 kernel
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
TAG=${TAG:-r02_e}
O=gpurun_out/$TAG
mkdir -p $O
timeout 1200 python -m pytest tests -m gpu -x -q > $O/pytest.log 2>&1; tail -4 $O/pytest.log
Q="--steps 5 --warmup 2 --cpu-sample 0 --latency-requests 0 --e2e-seconds 0"
show() { python - "$1" "$2" <<'PY'
import json, sys
try:
    d = json.load(open(sys.argv[2]))
    print(sys.argv[1], round(d['value']/1e6, 1), 'M items/s', round(d['ms_per_device_batch'], 3), 'ms/batch', {k: round(v['avg_ms'] * v['launches_per_batch'], 3) for k, v in d['kernels'].items()}, d['config'].get('scorer'))
except Exception as e:
    print(sys.argv[1], 'FAILED', e)
PY
}
timeout 600 python bench.py --full --workload c2 $Q > $O/c2.json 2> $O/c2.log; show "c2" $O/c2.json
timeout 600 python bench.py --full --workload c3 $Q > $O/c3.json 2> $O/c3.log; show "c3" $O/c3.json
timeout 900 python bench.py --full --workload c4x --clones 19 --items 2000000 $Q > $O/c4x.json 2> $O/c4x.log; show "c4x(2M of 2M)" $O/c4x.json
timeout 600 python bench.py --full --workload c2 --backend xgboost --trees 100 --depth 6 $Q > $O/c2_xgb_d6.json 2> $O/c2_xgb_d6.log; show "c2 xgb 100x d6" $O/c2_xgb_d6.json
timeout 600 python bench.py --full --workload c2 --backend xgboost --trees 100 --depth 8 $Q > $O/c2_xgb_d8.json 2> $O/c2_xgb_d8.log; show "c2 xgb 100x d8" $O/c2_xgb_d8.json
timeout 600 python bench.py --full --workload c2 --backend xgboost --trees 500 --depth 4 $Q > $O/c2_xgb_d4.json 2> $O/c2_xgb_d4.log; show "c2 xgb 500x d4 (bit-vector)" $O/c2_xgb_d4.json
env MRK_SCORER=walk timeout 600 python bench.py --full --workload c2 $Q > $O/c2_walk.json 2> $O/c2_walk.log; show "c2 lgbm, walk scorer forced" $O/c2_walk.json
MRK_DEFINES=MRK_PHASE_CLOCKS python -c "from metarank_amd import _native; _native.build(force=True)" > $O/phase_build.log 2>&1
MRK_DEFINES=MRK_PHASE_CLOCKS timeout 600 python tools/phase_clocks.py c2 > $O/phase_c2.txt 2>&1; tail -40 $O/phase_c2.txt
