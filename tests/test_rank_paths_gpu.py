"""GPU: which launches a batch's shape takes (csrc/rank_plan.hpp plan_rank / plan_values, applied by capi_rank.cpp) - counted from
the outside: the per-timer launch counts of the profile, the debug export of a batch's fused cells launch and the names of the
specialised kernels that were loaded.  Every result is the oracle's, bit for bit.  tests/test_launch_shapes_cpu.py pins the plan
itself; this file pins that the launches follow it.

MRK_RANK_JIT=1: a kernel that is not on disk is compiled and waited for, so that which specialised kernel ran (the loaded kernels'
names, the kernel id of the fused launch) does not depend on a background compile.  MRK_JIT_SIG=0: kernels keyed by the program
alone, so that the code objects `__graft_entry__.build()` ships next to the library for the stock Ranklens program are what runs
and nothing is compiled here (without them the test compiles five kernels, 10 - 20 s each, and still passes).  The launch counts
do not depend on the keying: tests/test_rank_one_gpu.py and tests/test_table_compact_gpu.py run the same paths keyed by the forest."""

import numpy as np
import pytest

from backends import HipBackend, OracleBackend
from test_rank_one_gpu import N_ITEMS, N_SESS, restore_env, same, with_env
from workloads import ranklens, synth

TIMERS = ("prepass", "assemble", "score", "sort", "rank_one", "rank_one_walk", "rank_values", "normalize")


@pytest.fixture(scope="module")
def world():
    saved = with_env({"MRK_RANK_JIT": "1", "MRK_JIT_SIG": "0"})
    cfg = ranklens.ranklens_config()
    orc, hip = OracleBackend(cfg, "xgboost"), HipBackend(cfg, "xgboost")
    try:
        for b in (orc, hip):
            ranklens.load_state(b, ranklens.generate_state(N_ITEMS, N_SESS))
        sample = ranklens.generate_requests(6, 100, N_ITEMS, N_SESS, seed=81)
        q = ranklens.column_quantiles(np.concatenate([orc.matrix(ev) for ev in sample]))
        blob = synth.synthetic_lgbm_model(n_trees=500, n_features=24, quantiles=q, cat_features=[7], cat_prob=0.05, missing="per_feature")
        orc.load_model(blob, 0)
        hip.load_model(blob, 0)
        assert hip.booster.info()["bitvector"] == 1
        hip.ctx.profile_enable(True)
        yield orc, hip
    finally:
        hip.ctx.profile_enable(False)
        hip.close()
        restore_env(saved)


def launched(hip, what):
    """-> (what()'s result, {timer: launches during what()} without the zeros)"""
    before = {t: hip.ctx.profile_get(t)[1] for t in TIMERS}
    out = what()
    hip.ctx.sync()
    return out, {t: n for t in TIMERS if (n := hip.ctx.profile_get(t)[1] - before[t])}


@pytest.mark.gpu
@pytest.mark.parametrize("n,want,kernel", [
    (1, {"rank_one": 1}, "mrk_jit_rank_one"),
    (128, {"rank_one": 1}, "mrk_jit_rank_one"),
    (129, {"assemble": 1, "score": 1, "sort": 1}, "mrk_jit_rank_cells_split"),           # one candidate too many: a workgroup per request, no pre-pass launch
    (1025, {"prepass": 1, "assemble": 1, "score": 1, "sort": 1}, "mrk_jit_assemble_cells"),   # past the fused kernel's 1 024: item-parallel
])
def test_one_request_through_mrk_rank(world, n, want, kernel):
    orc, hip = world
    ev = ranklens.generate_requests(1, n, N_ITEMS, N_SESS, seed=500 + n)[0]
    (_, s, o), got = launched(hip, lambda: hip.ranker.rerank("xgboost", ev, hip.booster))
    _, es, eo = orc.rerank(ev)
    assert same(s, es) and o.tolist() == eo.tolist()
    assert got == want
    assert kernel in hip.ranker.kernel_keys("xgboost")
    if n == 1025:
        assert "mrk_jit_prepass" in hip.ranker.kernel_keys("xgboost")


@pytest.mark.gpu
def test_prepared_batch_and_its_matrix(world):
    orc, hip = world
    reqs = ranklens.generate_requests(2, 3, N_ITEMS, N_SESS, seed=601)
    batch = hip.ranker.prepare("xgboost", reqs)
    try:
        _, got = launched(hip, lambda: (batch.run(hip.booster), batch.fetch()))
        assert got == {"assemble": 1, "score": 1, "sort": 1}
        info = batch.launch_info()
        # two requests: op-split workgroups (launch_shape.hpp), so the split kernel and its 8-byte entries
        assert (info["kernel"], info["entry_bytes"], info["threads"]) == (2, 8, 256) and info["lds"] > 0
        # the matrix on demand: one more assembly launch, into the f64 matrix
        (scores, order, mat), got = launched(hip, lambda: batch.fetch(matrix=True))
        assert got == {"assemble": 1}
        for r, ev in enumerate(reqs):
            em, es, eo = orc.rerank(ev)
            lo, hi = batch.offsets[r], batch.offsets[r + 1]
            assert same(scores[lo:hi], es) and order[lo:hi].tolist() == eo.tolist() and same(mat[lo:hi], em)
    finally:
        batch.close()


@pytest.mark.gpu
def test_values_run(world):
    orc, hip = world
    ev = ranklens.generate_requests(1, 3, N_ITEMS, N_SESS, seed=602)[0]
    saved = with_env({"MRK_RANK_JIT": "0"})   # (mrk_jit_rank_values is not among the shipped code objects: the interpreting kernel, no compiler)
    try:
        rows, got = launched(hip, lambda: hip.ranker.values(ev, model="xgboost", offline=False))
    finally:
        restore_env(saved)
    assert got == {"rank_values": 1}
    assert same(rows, orc.matrix(ev))
