"""mrk_rank's ONE-LAUNCH path for forests the bit-vector scorer does not take (csrc/rank_device.hpp rank_one_walk_body:
pre-pass + assembly into an LDS matrix + the tree walk of score.hip + ordering in the request's workgroup) against the
oracle and against the three launches it replaces (MRK_RANK_ONE_WALK=0): same scores, same order, same per-request errors,
specialised and interpreting kernel; the same model through both one-launch scorers (MRK_SCORER=walk); edge forests."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import metarank_amd as M
from backends import HipBackend, OracleBackend
from test_rank_one_gpu import N_ITEMS, N_SESS, requests, restore_env, same, with_env
from workloads import ranklens, synth

KERNEL = "rank_one_walk"   # the launch timer of the new kernel (mrk_profile_get)


def launches(hip) -> int:
    return hip.ctx.profile_get(KERNEL)[1]


def xgb_model(n_trees, depth, quantiles, cat=True, base_score=0.5, seed=synth.SEED):
    rng = np.random.Generator(np.random.PCG64(seed))
    trees = [synth.random_xgb_tree(rng, 24, depth, quantiles, [7] if cat else None, 0.05 if cat else 0.0, 16, True) for _ in range(n_trees)]
    return synth.write_xgboost_json(synth.xgboost_document(trees, 24, base_score=base_score))


def model_of(kind, q):
    if kind == "xgb6":   # 137 trees of depth 6, categorical splits on column 7, a base score that is not the default
        return xgb_model(137, 6, q, base_score=0.3125), 1
    if kind == "xgb8":
        return xgb_model(7, 8, q), 1
    if kind == "lgbm40":  # 40 leaves per tree, every split draws its own missing type
        return synth.synthetic_lgbm_model(n_trees=120, n_features=24, num_leaves=40, max_depth=10, quantiles=q, cat_features=[7], cat_prob=0.05, missing="per_node"), 0
    raise ValueError(kind)


def state_pair(cfg=None, c3=False):
    cfg = cfg or ranklens.ranklens_config()
    orc, hip = OracleBackend(cfg, "xgboost"), HipBackend(cfg, "xgboost")
    for b in (orc, hip):
        ranklens.load_state(b, ranklens.generate_state(N_ITEMS, N_SESS, c3=c3))
    return orc, hip


def sized_requests():
    reqs = requests()   # 6 x 100, 1, 128, 129, none, odd
    reqs += ranklens.generate_requests(1, 64, N_ITEMS, N_SESS, seed=87) + ranklens.generate_requests(1, 65, N_ITEMS, N_SESS, seed=88)
    return reqs


@pytest.mark.gpu
@pytest.mark.parametrize("jit", ["1", "0"])
@pytest.mark.parametrize("kind", ["xgb6", "xgb8", "lgbm40"])
def test_one_launch_equals_three_launches_and_the_oracle(kind, jit):
    saved = with_env({"MRK_RANK_JIT": jit, "MRK_RANK_ONE_WALK": "1"})   # mrk_rank takes the walking one-launch kernel when asked to (LOG.md round 10)
    orc, hip = state_pair()
    try:
        reqs = sized_requests()
        q = ranklens.column_quantiles(np.concatenate([orc.matrix(ev) for ev in reqs[:6]]))
        blob, backend = model_of(kind, q)
        orc.load_model(blob, backend)
        hip.load_model(blob, backend)
        assert hip.booster.info()["bitvector"] == 0
        hip.ctx.profile_enable(True)
        got, rose = {}, []
        for walk in ("1", "0"):
            s2 = with_env({"MRK_RANK_ONE_WALK": walk})
            got[walk] = []
            for ev in reqs:
                before = launches(hip)
                got[walk].append(hip.ranker.rerank("xgboost", ev, hip.booster))
                if walk == "1":
                    rose.append(launches(hip) - before)
            restore_env(s2)
        hip.ctx.profile_enable(False)
        for k, ev in enumerate(reqs):
            _, es, eo = orc.rerank(ev)
            for walk in ("1", "0"):
                _, s, o = got[walk][k]
                assert same(s, es) and o.tolist() == eo.tolist(), (kind, jit, walk, k)
            # the new kernel ran for every request of 1 ... 128 candidates and for none beyond (no candidates: nothing to launch)
            n = len(ev["items"])
            assert rose[k] == (1 if 1 <= n <= 128 else 0), (kind, jit, k, n, rose[k])
        # ... again and again: barrier and overlay mistakes show up once in many launches
        many = ranklens.generate_requests(60, 100, N_ITEMS, N_SESS, seed=1234)
        want = [orc.rerank(ev) for ev in many]
        for rep in range(3):
            for k, ev in enumerate(many):
                _, s, o = hip.ranker.rerank("xgboost", ev, hip.booster)
                assert same(s, want[k][1]) and o.tolist() == want[k][2].tolist(), (kind, jit, "repeat", rep, k)
        # concurrent callers: the batching front hands the kernel several requests at a time
        with ThreadPoolExecutor(12) as ex:
            res = list(ex.map(lambda ev: hip.ranker.rerank("xgboost", ev, hip.booster), reqs * 3))
        for k, (_, s, o) in enumerate(res):
            _, es, eo = got["0"][k % len(reqs)]
            assert same(s, es) and o.tolist() == eo.tolist(), k
    finally:
        restore_env(saved)
        hip.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lgbm16", "xgb4"])
def test_same_model_through_both_one_launch_scorers(kind):
    """A forest of 16-leaf trees: the bit-vector one-launch kernel (default) and the walking one (MRK_SCORER=walk) give the same bytes."""
    orc, hip = state_pair()
    try:
        reqs = sized_requests()
        q = ranklens.column_quantiles(np.concatenate([orc.matrix(ev) for ev in reqs[:6]]))
        if kind == "lgbm16":
            blob, backend = synth.synthetic_lgbm_model(n_trees=200, n_features=24, quantiles=q, cat_features=[7], cat_prob=0.05, missing="per_feature"), 0
        else:
            blob, backend = synth.synthetic_xgb_model(n_trees=137, n_features=24, depth=4, quantiles=q, cat_features=[7], cat_prob=0.05), 1
        hip.load_model(blob, backend)
        assert hip.booster.info()["bitvector"] == 1
        hip.ctx.profile_enable(True)
        base = [hip.ranker.rerank("xgboost", ev, hip.booster) for ev in reqs]
        assert launches(hip) == 0
        saved = with_env({"MRK_SCORER": "walk", "MRK_RANK_ONE_WALK": "1"})
        try:
            walk = [hip.ranker.rerank("xgboost", ev, hip.booster) for ev in reqs]
        finally:
            restore_env(saved)
        assert launches(hip) == sum(1 for ev in reqs if 1 <= len(ev["items"]) <= 128)
        for k in range(len(reqs)):
            assert base[k][1].tobytes() == walk[k][1].tobytes() and base[k][2].tolist() == walk[k][2].tolist(), (kind, k)
    finally:
        hip.close()


@pytest.mark.gpu
def test_errors_are_the_three_launch_path_s():
    orc, hip = state_pair()
    try:
        evs = ranklens.generate_requests(5, 50, N_ITEMS, N_SESS, seed=85)
        hip.load_model(xgb_model(20, 6, None, cat=False), 1)
        assert hip.booster.info()["bitvector"] == 0
        # inside a combined batch only the offending request fails
        bad_item = evs[2]["items"][3]["id"]
        clean = [ev for ev in evs if all(it["id"] != bad_item for it in ev["items"])]
        assert evs[2] not in clean and len(clean) >= 2
        want = [hip.ranker.rerank("xgboost", ev, hip.booster) for ev in clean]
        hip.put_double(f"item={bad_item}/popularity", 1e300)   # +inf after the Double -> Float narrowing
        hip.ctx.profile_enable(True)
        for walk in ("1", "0"):
            saved = with_env({"MRK_RANK_ONE_WALK": walk})
            with pytest.raises(M.MrkError) as ei:
                hip.ranker.rerank("xgboost", evs[2], hip.booster)
            assert ei.value.status == -1 and "inf" in ei.value.message, walk

            def call(ev):
                try:
                    return hip.ranker.rerank("xgboost", ev, hip.booster)
                except M.MrkError as e:
                    return e
            with ThreadPoolExecutor(8) as ex:
                res = list(ex.map(call, (clean + [evs[2]]) * 4))
            for k, r in enumerate(res):
                j = k % (len(clean) + 1)
                if j == len(clean):
                    assert isinstance(r, M.MrkError) and r.status == -1, (walk, k)
                else:
                    assert not isinstance(r, M.MrkError) and same(r[1], want[j][1]) and r[2].tolist() == want[j][2].tolist(), (walk, k)
            restore_env(saved)
        assert launches(hip) > 0
        # a request the reference throws on (normalised rate: global clicks == 0)
        hip.put_periodic("global/ctr_click_norm", [0, 5])
        for walk in ("1", "0"):
            saved = with_env({"MRK_RANK_ONE_WALK": walk})
            before = launches(hip)
            with pytest.raises(M.MrkError) as ei:
                hip.ranker.rerank("xgboost", clean[0], hip.booster)
            assert ei.value.status == -5, walk
            assert launches(hip) - before == (1 if walk == "1" else 0), walk   # the error came out of the kernel under test
            restore_env(saved)
    finally:
        hip.close()


def lgbm_with_stump(q):
    """a LightGBM forest of 40-leaf trees whose third tree is a single leaf"""
    rng = np.random.Generator(np.random.PCG64(5))
    trees = [synth.random_lgbm_tree(rng, 24, 40, 10, q) for _ in range(9)]
    stump = synth.random_lgbm_tree(rng, 24, 1, 1, q)
    return synth.write_lightgbm_text(trees[:2] + [stump] + trees[2:], 24)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["one_tree", "stump", "chunks"])
def test_edge_forests(kind):
    saved = with_env({"MRK_RANK_ONE_WALK": "1"})
    orc, hip = state_pair()
    try:
        reqs = sized_requests()
        q = ranklens.column_quantiles(np.concatenate([orc.matrix(ev) for ev in reqs[:6]]))
        if kind == "one_tree":
            blob, backend = xgb_model(1, 7, q), 1
        elif kind == "stump":
            blob, backend = lgbm_with_stump(q), 0
        else:   # depth 8: 255 nodes x 16 B + 256 leaves x 4 B = 5 104 B a tree, four to a 24 KB chunk: 14 trees are 4 chunks
            blob, backend = xgb_model(14, 8, q), 1
        orc.load_model(blob, backend)
        hip.load_model(blob, backend)
        info = hip.booster.info()
        assert info["bitvector"] == 0
        if kind == "chunks":
            # chunks hold whole trees within score.hip's 24 KB budget; the 14 complete trees are equal, so a tree's bytes (16 B a node, 4 B
            # a leaf) say how many fit: at most 4 (five would pass 24 KB) - 14 trees are then at least 4 chunks
            assert info["n_trees"] == 14 and (info["n_nodes"] * 16 + info["n_leaves"] * 4) / 14 * 5 > 24 * 1024, info
        hip.ctx.profile_enable(True)
        for k, ev in enumerate(reqs):
            _, es, eo = orc.rerank(ev)
            _, s, o = hip.ranker.rerank("xgboost", ev, hip.booster)
            assert same(s, es) and o.tolist() == eo.tolist(), (kind, k)
        assert launches(hip) == sum(1 for ev in reqs if 1 <= len(ev["items"]) <= 128)
    finally:
        restore_env(saved)
        hip.close()


@pytest.mark.gpu
def test_a_model_whose_matrix_does_not_fit_keeps_three_launches():
    """64 f64 columns x 128 rows are 64 KB: with a 24 KB chunk next to them the kernel's LDS passes 96 KB."""
    cfg = ranklens.c3_config()
    saved = with_env({"MRK_RANK_ONE_WALK": "1"})
    orc, hip = state_pair(cfg, c3=True)
    try:
        reqs = ranklens.generate_requests(3, 100, N_ITEMS, N_SESS, seed=81)
        dim = hip.dim
        assert dim == 64
        q = ranklens.column_quantiles(np.concatenate([orc.matrix(ev) for ev in reqs]))
        blob = synth.synthetic_lgbm_model(n_trees=80, n_features=dim, num_leaves=40, max_depth=10, quantiles=q, missing="per_node")
        orc.load_model(blob, 0)
        hip.load_model(blob, 0)
        assert hip.booster.info()["bitvector"] == 0
        hip.ctx.profile_enable(True)
        for k, ev in enumerate(reqs):
            _, es, eo = orc.rerank(ev)
            _, s, o = hip.ranker.rerank("xgboost", ev, hip.booster)
            assert same(s, es) and o.tolist() == eo.tolist(), k
        assert launches(hip) == 0 and hip.ctx.profile_get("score")[1] >= len(reqs)
    finally:
        restore_env(saved)
        hip.close()
