"""The serving queue (mrk_serve_*: persistent workgroups polling slots in pinned memory) for forests the bit-vector scorer does
not take - trees of more than 16 leaves, walked in the request's workgroup (csrc/rank_device.hpp rank_serve_walk_body): the
queue starts, every answer equals mrk_batch_run's on the same requests, mrk_rank answers through the started queue, the
statistics count the requests, the queue stops; a model whose matrix cannot fit the workgroup's LDS is refused by name."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import metarank_amd as M
from backends import HipBackend, OracleBackend
from test_rank_one_gpu import N_ITEMS, N_SESS, restore_env, same, with_env
from test_rank_one_walk_gpu import model_of
from workloads import ranklens, synth

SIZES = [0, 1, 2, 7, 31, 63, 64, 65, 100, 127, 128]


def mixed_requests(n):
    out = []
    for k in range(n):
        size = SIZES[k % len(SIZES)]
        if size == 0:
            out.append({"id": f"none{k}", "timestamp": ranklens.TS, "user": None, "session": None, "fields": [], "items": []})
        else:
            out += ranklens.generate_requests(1, size, N_ITEMS, N_SESS, seed=500 + k)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("jit", ["1", "0"])   # the specialised persistent kernel (mrk_jit_rank_serve_walk) and the interpreting one
@pytest.mark.parametrize("kind", ["xgb6", "lgbm40"])
def test_serving_queue_takes_deep_forests(kind, jit):
    saved = with_env({"MRK_RANK_JIT": jit})
    cfg = ranklens.ranklens_config()
    orc, hip = OracleBackend(cfg, "xgboost"), HipBackend(cfg, "xgboost")
    srv = None
    try:
        for b in (orc, hip):
            ranklens.load_state(b, ranklens.generate_state(N_ITEMS, N_SESS))
        evs = mixed_requests(200)
        q = ranklens.column_quantiles(np.concatenate([orc.matrix(ev) for ev in evs[8:11]]))
        blob, backend = model_of(kind, q)
        hip.load_model(blob, backend)
        assert hip.booster.info()["bitvector"] == 0
        # the expected bytes: mrk_batch_run on the same requests
        batch = hip.ranker.prepare("xgboost", evs)
        batch.run(hip.booster)
        scores, order, _ = batch.fetch()
        want = [(scores[batch.offsets[r]:batch.offsets[r + 1]].copy(), order[batch.offsets[r]:batch.offsets[r + 1]].copy()) for r in range(len(evs))]
        batch.close()
        reqs = [M.Request(ev) for ev in evs]
        srv = hip.ranker.serve("xgboost", hip.booster, n_slots=8)   # fails with MRK_ERR_UNSUPPORTED before the walking workgroup existed
        with ThreadPoolExecutor(8) as ex:
            res = list(ex.map(srv.rerank, reqs))
        for k, (s, o) in enumerate(res):
            assert same(s, want[k][0]) and o.tolist() == want[k][1].tolist(), (kind, jit, k, len(evs[k]["items"]))
        st = srv.stats()
        # 8 callers on 8 slots, every request of at most 128 candidates and without overrides: all of them through the queue
        assert st["queue"] == len(evs) and st["fallback"] == 0 and st["launches"] >= 1, st
        if jit == "1":
            assert "mrk_jit_rank_serve_walk" in hip.ranker.kernel_keys("xgboost"), hip.ranker.kernel_keys("xgboost")
        # mrk_rank, called while the queue is started, is answered through it
        for k in (8, 9, 10):
            _, s, o = hip.ranker.rerank("xgboost", reqs[k], hip.booster)
            assert same(s, want[k][0]) and o.tolist() == want[k][1].tolist(), k
        assert srv.stats()["queue"] == st["queue"] + 3
        srv.close()
        srv = None
        # same-build A/B switch: the queue refuses the model as it did before
        s2 = with_env({"MRK_RANK_ONE_WALK": "0"})
        try:
            with pytest.raises(M.MrkError) as ei:
                hip.ranker.serve("xgboost", hip.booster, n_slots=1)
            assert ei.value.status == -6
        finally:
            restore_env(s2)
    finally:
        if srv is not None:
            srv.close()
        restore_env(saved)
        hip.close()


@pytest.mark.gpu
def test_a_model_that_cannot_fit_is_refused_with_the_limit():
    """136 f64 columns x 128 rows are 139 264 B of matrix: more than the serving workgroup's 128 KB before any chunk."""
    cfg = ranklens.ranklens_config()
    extra = [{"name": f"y{i}", "type": "number", "scope": "item", "source": f"metadata.y{i}"} for i in range(112)]
    cfg["features"] += extra
    cfg["models"]["xgboost"]["features"] += [f["name"] for f in extra]
    hip = HipBackend(cfg, "xgboost")
    try:
        assert hip.dim == 136
        hip.load_model(synth.synthetic_lgbm_model(n_trees=5, n_features=136, num_leaves=40, max_depth=10), 0)
        assert hip.booster.info()["bitvector"] == 0
        with pytest.raises(M.MrkError) as ei:
            hip.ranker.serve("xgboost", hip.booster, n_slots=1)
        assert ei.value.status == -6
        msg = ei.value.message
        assert "136 columns" in msg and "8 bytes" in msg and "chunk" in msg and "131072" in msg, msg
    finally:
        hip.close()
