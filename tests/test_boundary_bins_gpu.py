"""GPU: every binning path on threshold-adjacent values (tests/boundary_forests.py), bit for bit against the numpy reference
evaluator and the oracle.

The device computes bin(x) in four separately written searches - qs_bin_search (run-time loop, global memory),
qs_bin_search_staged (fixed steps over 128-entry chunks in LDS), CellSinkRT::bin_group (interleaved searches over the
resident compact tables) - and the byte-mode scorer clamps the cell (v_pk_min_u16 to 255).  The forests here are decodable:
a single-column probe's score IS its bin, so a failure names the column, the probe value and both bins.

Figures of the committed seeds (rows = single-column probes + 320 dense rows; LightGBM | XGBoost):
  layout S: 24 | 25 split-on columns of 27 | 28, tables of 1 .. 65 entries, 2 339 | 5 336 probe rows
  layout M: 26 | 27 of 29 | 30, tables of 1 .. 255 (127/128/129, 191/192/193, 253/254/255), 7 171 | 19 748 rows (and per-tree rules)
  layout L: 23 | 24 of 26 | 27, tables of 1 .. 520 (256, 257, 300, 520), 10 663 | 30 341 rows
"""
import os

import numpy as np
import pytest

import boundary_forests as bf
import metarank_amd as M
from backends import HipBackend
from metarank_amd.request import Request
from oracle.assembly import sort_order
from oracle.forest import OracleForest

pytestmark = pytest.mark.gpu

SCORER_KEYS = ("MRK_SCORER", "MRK_QS_KERNEL", "MRK_QS_R", "MRK_QS_SPLIT", "MRK_WALK_TILE", "MRK_QS_BYTE")
RANK_KEYS = ("MRK_RANK_FUSED", "MRK_RANK_CELLS", "MRK_RANK_JIT", "MRK_JIT_SIG", "MRK_ITEMS_RT", "MRK_FUSED_SPLIT", "MRK_JIT_DEFINES")
STAGE = "MRK_FUSED_RT_MAX=0 MRK_FUSED_RT_MAX_SPLIT=0"   # the staging sink where the tables would be resident


@pytest.fixture
def env_restored():
    saved = {k: os.environ.get(k) for k in SCORER_KEYS + RANK_KEYS}
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    M.reload_switches()


def set_env(keys, **env):
    for k in keys:
        os.environ.pop(k, None)
    os.environ.update({k: v for k, v in env.items() if v is not None})
    M.reload_switches()


def oracle_scores(f, X):
    blob = f.model_bytes()
    return (OracleForest.from_xgboost(blob) if f.is_xgb else OracleForest.from_lightgbm_text(blob)).predict(X)


def scorer_variants():
    out = [(f"bitvector-wave-split{nw}", dict(MRK_QS_KERNEL="1", MRK_QS_SPLIT=nw)) for nw in ("1", "2", "4", "8", "16")]
    out.append(("bitvector-wave-auto", dict(MRK_QS_KERNEL="1")))
    out += [(f"bitvector-generic-r{r}", dict(MRK_QS_KERNEL="0", MRK_QS_R=r)) for r in ("2", "4", "8")]
    out += [("walk", dict(MRK_SCORER="walk")), ("walk-256-row-tiles", dict(MRK_SCORER="walk", MRK_WALK_TILE="256"))]
    return out


# --------------------------------------------------------------------------------------------- Booster.predictMat
@pytest.mark.parametrize("layout,backend,rules", bf.CASES)
def test_predict_every_scorer_on_the_boundary_grid(ctx, env_restored, layout, backend, rules):
    f, X, meta, ref = bf.case(layout, backend, rules)
    assert np.array_equal(oracle_scores(f, X), ref)
    b = M.HipBooster(f.model_bytes(), M.XGBOOST if f.is_xgb else M.LIGHTGBM, ctx)
    try:
        assert b.info()["bitvector"] == 1 and b.info()["n_trees"] == len(f.trees)
        rng = np.random.default_rng(len(X))
        subsets = [np.arange(len(X))] + [np.sort(rng.choice(len(X), n, replace=False)) for n in (1, 127, 128, 129)]
        assert len(X) % 128 != 0 and len(X) > 1000
        byte_modes = (None, "0") if layout in ("S", "M") else (None,)   # byte-eligible by construction: on (default) and off
        ran = []
        for byte in byte_modes:
            for name, env in scorer_variants():
                for rows in subsets:
                    set_env(SCORER_KEYS, MRK_QS_BYTE=byte, **env)
                    got = b.predict(X[rows])
                    label = f"{name}, MRK_QS_BYTE={byte or 'default'}, {len(rows)} rows"
                    assert np.array_equal(got, ref[rows]), label + "\n" + f.explain(X[rows], [meta[r] for r in rows], got, ref[rows])
                ran.append(name)
        print(f"{backend} {layout} {rules}: {len(X)} probe rows, tables {sorted(set(f.lengths.values()))}, "
              f"{len(ran)} scorer runs x {len(subsets)} row counts")
    finally:
        b.close()


# --------------------------------------------------------------------------------------------- the /rank path
def rank_config(n_cols):
    names = [f"c{j}" for j in range(n_cols)]
    return {"features": [{"name": n, "type": "number", "scope": "item", "source": f"metadata.{n}"} for n in names],
            "models": {"m": {"type": "lambdamart", "backend": {"type": "lightgbm", "iterations": 10}, "features": names}}}


def put_rows(hip, X, prefix="p"):
    """item `prefix``r` = row r; a NaN cell is a field left unset (it must read as NaN)"""
    for r in range(len(X)):
        for c in range(X.shape[1]):
            if not np.isnan(X[r, c]):
                hip.put_double(f"item={prefix}{r}/c{c}", X[r, c])


def event(name, ids):
    return {"id": name, "timestamp": 1661345221008, "user": None, "session": None, "fields": [], "items": [{"id": i} for i in ids]}


def same_matrix(got, exp):
    """bitwise (as u64) wherever the probe is a number - -0.0 and the denormals included - NaN where it is NaN"""
    n = np.isnan(exp)
    return got.shape == exp.shape and bool((np.isnan(got) == n).all()) and bool((bf.bits(got)[~n] == bf.bits(exp)[~n]).all())


# (name, environment): every assembly path tests/test_rank_parity.py::test_assembly_paths_agree switches
def assembly_paths():
    out = []
    for fused, cells, jit, sig in (("1", "1", "require", "1"), ("1", "1", "require", "0"), ("1", "1", "0", "1"), ("1", "0", "require", "1"), ("1", "0", "0", "1"),
                                   ("0", "1", "require", "1"), ("0", "1", "require", "0"), ("0", "1", "0", "1"), ("0", "0", "0", "1")):
        out.append((f"fused={fused} cells={cells} jit={jit} sig={sig}", dict(MRK_RANK_FUSED=fused, MRK_RANK_CELLS=cells, MRK_RANK_JIT=jit, MRK_JIT_SIG=sig)))
    for fused, split, defs, items_rt in (("1", None, STAGE, "1"), ("1", "2", STAGE, "1"), ("1", "2", None, "1"), ("0", None, None, "0"), ("0", None, "MRK_RT_Q=2", "1")):
        out.append((f"sink: fused={fused} split={split} defines={defs} items_rt={items_rt}",
                    dict(MRK_RANK_FUSED=fused, MRK_RANK_CELLS="1", MRK_RANK_JIT="require", MRK_JIT_SIG="1", MRK_ITEMS_RT=items_rt, MRK_FUSED_SPLIT=split, MRK_JIT_DEFINES=defs)))
    return out


@pytest.mark.parametrize("layout,backend,rules", bf.CASES)
def test_rank_every_assembly_path_on_the_boundary_grid(env_restored, layout, backend, rules):
    f, X, meta, ref = bf.case(layout, backend, rules)
    assert np.array_equal(oracle_scores(f, X), ref)
    n = len(X)
    hip = HipBackend(rank_config(f.n_cols), "m")
    try:
        assert hip.dim == f.n_cols
        put_rows(hip, X)
        hip.load_model(f.model_bytes(), 1 if f.is_xgb else 0)
        assert hip.booster.info()["bitvector"] == 1
        # requests of 1, 100 and 300 items, one beyond the single-workgroup sort (the sample sort), then every remaining row
        big = 5000
        spans = [np.arange(0, 1), np.arange(1, 101), np.arange(101, 401), np.arange(401, 401 + big) % n]
        spans += [np.arange(lo, min(lo + 300, n)) for lo in range(401, n, 300)]
        assert set(np.concatenate(spans).tolist()) == set(range(n))
        reqs = [Request(event(f"r{k}", [f"p{r}" for r in rows])) for k, rows in enumerate(spans)]
        expected = [(ref[rows], sort_order(ref[rows])) for rows in spans]

        def check(label, k, rows, scores, order, mat=None):
            es, eo = expected[k]
            if mat is not None:
                assert same_matrix(mat, X[rows]), f"{label}: request {k}: the fetched matrix is not the probe matrix"
            assert np.array_equal(scores, es), f"{label}: request {k}\n" + f.explain(X[rows], [meta[r] for r in rows], scores, es)
            assert order.tolist() == eo.tolist(), f"{label}: request {k}: order"

        ran = []
        for label, env in assembly_paths():
            set_env(RANK_KEYS, **env)
            batch = hip.ranker.prepare("m", reqs)
            try:
                batch.run(hip.booster)
            except M.MrkError as e:   # a combination the library rejects is named, not skipped silently
                batch.close()
                pytest.fail(f"{label}: rejected by the library: {e}")
            scores, order, mat = batch.fetch(matrix=True)
            assert (batch.status() == 0).all(), label
            for k, rows in enumerate(spans):
                lo, hi = batch.offsets[k], batch.offsets[k + 1]
                check(label, k, rows, scores[lo:hi], order[lo:hi], mat[lo:hi])
            batch.close()
            ran.append(label)
        # mrk_rank, one request at a time (the one-launch kernel for the small ones), without and with the matrix
        set_env(RANK_KEYS, MRK_RANK_FUSED="1", MRK_RANK_CELLS="1", MRK_RANK_JIT="require")
        for k in (0, 1, 2, 3):
            _, s, o = hip.ranker.rerank("m", reqs[k], hip.booster, explain=False)
            check("mrk_rank", k, spans[k], s, o)
            m, s, o = hip.ranker.rerank("m", reqs[k], hip.booster, explain=True)
            check("mrk_rank explain", k, spans[k], s, o, m)
        print(f"{backend} {layout} {rules}: {n} probe rows in {len(reqs)} requests; paths: " + "; ".join(ran) + "; mrk_rank")
    finally:
        hip.close()


def test_rank_xgboost_inf_fails_its_request_alone_through_every_sink(env_restored):
    """A value that narrows to inf - in a split-on column, in a never-split column, in the column beyond num_feature - gives
    its request the inf status through every sink; the other requests of the batch keep status 0 and correct scores."""
    f, X, meta, ref = bf.case("S", "xgb")
    hip = HipBackend(rank_config(f.n_cols), "m")
    try:
        good = np.arange(0, len(X), max(1, len(X) // 240))[:240]
        put_rows(hip, X[good])                       # items p0 .. p239
        where = {"split": f.split_cols[3], "unsplit": f.unsplit_cols[0], "beyond": f.num_feature}
        for name, c in where.items():
            row = np.full((1, f.n_cols), f.neutral)
            row[0, c] = 3.5e38                       # finite in f64, inf after the Double -> Float narrowing
            assert np.isinf(bf.f32(row[0, c]))
            put_rows(hip, row, prefix=f"inf_{name}_")
        hip.load_model(f.model_bytes(), 1)
        ids = [f"p{k}" for k in range(len(good))]
        reqs, bad = [], {}
        for k, name in enumerate(where):
            reqs.append(event(f"ok{k}", ids[80 * k:80 * k + 80]))
            bad[len(reqs)] = name
            reqs.append(event(f"bad_{name}", ids[:40] + [f"inf_{name}_0"] + ids[40:70]))
        reqs.append(event("ok_last", ids[::-1]))
        rows_of = {0: good[0:80], 2: good[80:160], 4: good[160:240], 6: good[::-1]}
        for label, env in assembly_paths():
            set_env(RANK_KEYS, **env)
            batch = hip.ranker.prepare("m", reqs)
            batch.run(hip.booster)
            st = batch.status()
            scores, order, _ = batch.fetch()
            for k in range(len(reqs)):
                if k in bad:
                    assert st[k] == -1, f"{label}: inf in the {bad[k]} column: status {st[k]}"
                else:
                    assert st[k] == 0, f"{label}: request {k}: status {st[k]}"
                    lo, hi = batch.offsets[k], batch.offsets[k + 1]
                    es = ref[rows_of[k]]
                    assert np.array_equal(scores[lo:hi], es), f"{label}: request {k}\n" + f.explain(X[rows_of[k]], [meta[r] for r in rows_of[k]], scores[lo:hi], es)
                    assert order[lo:hi].tolist() == sort_order(es).tolist(), f"{label}: request {k}: order"
            batch.close()
        set_env(RANK_KEYS, MRK_RANK_JIT="require")
        for name in where:   # mrk_rank: the one-launch kernel reports it too
            with pytest.raises(M.MrkError) as e:
                hip.ranker.rerank("m", event("one", ids[:5] + [f"inf_{name}_0"]), hip.booster)
            assert e.value.status == -1 and "inf" in e.value.message, name
    finally:
        hip.close()
