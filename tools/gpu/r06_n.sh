# r06_n: compact resident threshold tables in the workgroup-per-request kernel (CellSinkRT in mrk_jit_rank_cells): the GPU suite,
# same-box A/B against ab/base (the staging sink) on c2 / c3 / c4x / c5, diversity group 4 vs 8, phase clocks
O=gpurun_out/r06_n; mkdir -p $O
F='^RCCL\|^HIP version\|^ROCm\|^Hostname\|^Librccl'
export MRK_RANK_JIT=1
timeout 1500 python -m pytest tests -m gpu -x -q 2>&1 | grep -E "passed|failed|error|Error" | tail -5 | tee $O/pytest_gpu.log
for wl in c2 c4x c3; do
for v in "MRK_LIB=$PWD/ab/base/libmrk_hip.so MRK_JIT_DEFINES=MRK_GET_K=1" "MRK_X=1" "MRK_JIT_DEFINES=MRK_DIV_GROUP=8" "MRK_LIB=$PWD/ab/base/libmrk_hip.so MRK_JIT_DEFINES=MRK_GET_K=1" "MRK_X=1"; do
  env $v timeout 600 python bench.py --full --workload $wl --steps 5 --warmup 2 --cpu-sample 0 --latency-requests 100 --latency-sweep 0 --e2e-seconds 0 --concurrent-callers '' 2>$O/$wl.log | python -c "
import json,sys
d=json.loads(sys.stdin.read()); print('$wl ${v:0:24}', round(d['value']/1e6,1), 'M items/s', {k: round(x['avg_ms'],4) for k,x in d['kernels'].items()}, 'p50', (d.get('latency') or {}).get('p50_ms'))"
done
done | tee $O/ab.txt
export MRK_LIB=$PWD/ab/clk/libmrk_hip.so MRK_BENCH_PHASE=1
timeout 300 python tools/phase_clocks.py c2 32 2>&1 | grep -v "$F" | tee $O/clk_c2_unloaded.txt
