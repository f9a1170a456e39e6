"""GPU: the LambdaMART fit (mrk_train_*, csrc/train.hip) against its restatement (tests/train_reference.py): gradients as bit patterns,
models as bytes, no tolerances.  The restatement is checked against itself and the oracle's reader in tests/test_train_cpu.py."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import eval_reference as E
import train_reference as T
import metarank_amd as M
from metarank_amd import _native
from metarank_amd.eval import evaluate
from metarank_amd.train import fit_lambdamart, lambdarank_gradients
from oracle.forest import OracleForest

pytestmark = pytest.mark.gpu

# csrc/train.hpp: TRAIN_BIN_ROWS = 256 rows per workgroup of the binning kernel, TRAIN_HIST_ROWS = 2048 of the histogram kernel
TILE_ROWS = [255, 256, 257, 2047, 2048, 2049]
SIZES = [1, 2, 63, 64, 65, 257, 4096]
TRUNCATIONS = [1, 30, 5000]


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ gradients
@functools.lru_cache(maxsize=None)
def grad_groups():
    """per size (scores, labels): scores rounded to one decimal (ties), +-100 in the larger groups (beyond the table's clamp)"""
    rng = np.random.default_rng(5)
    out = {}
    for n in SIZES:
        s = np.round(rng.normal(size=n) * 2.0, 1)
        if n >= 63:
            s[rng.integers(0, n, 3)] = 100.0
            s[rng.integers(0, n, 3)] = -100.0
        out[n] = (s, rng.integers(0, 5, n).astype(np.float64))
    out["equal"] = (np.round(rng.normal(size=10), 1), np.full(10, 2.0))
    out["zeros"] = (np.round(rng.normal(size=70), 1), np.zeros(70))
    return out


@functools.lru_cache(maxsize=None)
def grad_reference(key, truncation):
    s, y = grad_groups()[key]
    return T.gradients(s, y, [0, len(s)], 1.0, truncation)


@pytest.mark.parametrize("truncation", TRUNCATIONS)
def test_gradients_each_group_alone_and_all_shuffled_into_one_call(ctx, truncation):
    groups = grad_groups()
    for key, (s, y) in groups.items():
        g, h = lambdarank_gradients(s, y, [0, len(s)], ctx=ctx, truncation=truncation)
        eg, eh = grad_reference(key, truncation)
        assert np.array_equal(T.bits(g), T.bits(eg)) and np.array_equal(T.bits(h), T.bits(eh)), key
        if key in ("equal", "zeros", 1):
            assert not g.any() and not h.any()
    keys = list(groups)
    np.random.default_rng(truncation).shuffle(keys)
    s = np.concatenate([groups[k][0] for k in keys])
    y = np.concatenate([groups[k][1] for k in keys])
    off = np.concatenate([[0], np.cumsum([len(groups[k][0]) for k in keys])])
    g, h = lambdarank_gradients(s, y, off, ctx=ctx, truncation=truncation)
    eg = np.concatenate([grad_reference(k, truncation)[0] for k in keys])
    eh = np.concatenate([grad_reference(k, truncation)[1] for k in keys])
    assert np.array_equal(T.bits(g), T.bits(eg)) and np.array_equal(T.bits(h), T.bits(eh))
    assert g.any() and (h >= 0).all()


def test_gradients_refuse_a_group_of_4097_rows(ctx):
    with pytest.raises(_native.MrkError) as e:
        lambdarank_gradients(np.zeros(4097), np.zeros(4097), [0, 4097], ctx=ctx)
    assert e.value.status == _native.ERR_UNSUPPORTED and "4097" in e.value.message


# ------------------------------------------------------------------ models
def first_difference(got: bytes, want: bytes) -> str:
    tree = None
    gl, wl = got.decode().split("\n"), want.decode().split("\n")
    for i, (a, b) in enumerate(zip(gl, wl)):
        if a.startswith("Tree="):
            tree = a
        if a != b:
            return f"{tree}, line {i}:\n  device {a[:300]}\n  wanted {b[:300]}"
    return f"{len(gl)} lines against {len(wl)}"


def same_model(got: bytes, want: bytes):
    assert got == want, first_difference(got, want)


@functools.lru_cache(maxsize=None)
def reference_fit(rows, cfg_json, valid_rows=0, seed=1):
    X, y, off = T.dataset(seed, rows=rows)
    valid = T.dataset(100 + seed, rows=valid_rows) if valid_rows else None
    return T.fit(X, y, off, valid=valid, cfg=json.loads(cfg_json))


def both(ctx, rows, cfg, valid_rows=0, seed=1):
    X, y, off = T.dataset(seed, rows=rows)
    valid = T.dataset(100 + seed, rows=valid_rows) if valid_rows else None
    booster, hist = fit_lambdamart(X, y, off, valid=valid, ctx=ctx, **cfg)
    return booster, hist, reference_fit(rows, json.dumps(cfg, sort_keys=True), valid_rows, seed), X


def test_one_split_and_none(ctx):
    X, y, off = T.dataset(2, rows=200)
    X = X[:, [2, 3, 4]]
    cfg = {"numLeaves": 2, "iterations": 1, "sampling": 1.0}
    booster, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    want = T.fit(X, y, off, cfg=cfg)
    assert want["iterations_run"] == 1 and want["trees"][0].num_leaves == 2
    same_model(hist["model"], want["model"])
    assert hist["iterations_run"] == 1 and hist["best_iteration"] == 1
    booster.close()
    cfg["min_data_in_leaf"] = 101
    booster, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    want = T.fit(X, y, off, cfg=cfg)
    assert booster is None and hist["iterations_run"] == 0 and want["iterations_run"] == 0
    same_model(hist["model"], want["model"])
    assert not hist["scores"].any()


TREE_CASES = {
    "16 leaves": {"numLeaves": 16},
    "31 leaves": {"numLeaves": 31},
    "depth 3": {"numLeaves": 16, "maxDepth": 3},
    "half the columns": {"sampling": 0.5, "seed": 3},
    "half the columns, another seed": {"sampling": 0.5, "seed": 4},
    "lambda_l2": {"lambda_l2": 1.0},
}


@pytest.mark.parametrize("name", list(TREE_CASES))
def test_trees(ctx, name):
    cfg = dict(TREE_CASES[name], iterations=5)
    booster, hist, want, X = both(ctx, 3000, cfg)
    assert want["iterations_run"] == 5 and all(t.num_leaves > 2 for t in want["trees"])
    if name == "depth 3":
        assert all(t.num_leaves <= 8 and max(t.depth.values()) == 3 for t in want["trees"])
    if name == "31 leaves":
        assert max(t.num_leaves for t in want["trees"]) > 16
    same_model(hist["model"], want["model"])
    assert np.array_equal(T.bits(hist["scores"]), T.bits(want["scores"]))
    if name in ("16 leaves", "31 leaves"):
        # both scorer families read a trained forest: the bit-vector scorer (<= 16 leaves) and the tree walk
        got = booster.predict(X)
        assert np.array_equal(T.bits(got), T.bits(hist["scores"]))
        assert np.array_equal(T.bits(OracleForest.from_lightgbm_text(hist["model"]).predict(X)), T.bits(hist["scores"]))
        w = booster.weights(X.shape[1])                   # split_gain is written: Booster.weights() works
        assert w.shape == (X.shape[1],) and w[0] == 0.0 and w.sum() > 0.0   # (column 0 is constant: never split on)
    booster.close()


@pytest.mark.parametrize("rows", TILE_ROWS)
def test_row_counts_on_both_sides_of_the_tiles(ctx, rows):
    cfg = {"iterations": 2, "min_data_in_leaf": 5}
    booster, hist, want, _ = both(ctx, rows, cfg)
    assert want["iterations_run"] == 2
    same_model(hist["model"], want["model"])
    assert np.array_equal(T.bits(hist["scores"]), T.bits(want["scores"]))
    booster.close()


def test_cells_at_a_bound_and_one_ulp_beside_it(ctx):
    """T.adjacent: column 3 holds 1.0 - a bound, and the threshold the labels ask for - and its two neighbours one ulp away, through
    the binning kernel, the fit and both readers"""
    X, y, off = T.adjacent(3)
    cfg = {"iterations": 4, "min_data_in_leaf": 5}
    booster, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    want = T.fit(X, y, off, cfg=cfg)
    assert 1.0 in {t.thr[n] for t in want["trees"] for n in range(len(t.feat)) if t.feat[n] == 3}
    same_model(hist["model"], want["model"])
    assert np.array_equal(T.bits(hist["scores"]), T.bits(want["scores"]))
    assert np.array_equal(T.bits(booster.predict(X)), T.bits(hist["scores"]))
    booster.close()


def test_early_stopping(ctx):
    """seed 4, chosen on the CPU: with early_stopping = 3 the restatement stops after 8 of 40 iterations and keeps 5"""
    cfg = {"iterations": 40, "early_stopping": 3, "learningRate": 0.3, "min_data_in_leaf": 5}
    booster, hist, want, X = both(ctx, 1500, cfg, valid_rows=600, seed=4)
    assert want["iterations_run"] < 40 and want["best_iteration"] < want["iterations_run"]
    assert hist["iterations_run"] == want["iterations_run"] and hist["best_iteration"] == want["best_iteration"]
    assert np.array_equal(T.bits(hist["metric"]), T.bits(want["history"]))
    same_model(hist["model"], want["model"])
    assert hist["model"].count(b"Tree=") == want["best_iteration"]
    assert np.array_equal(T.bits(hist["scores"]), T.bits(want["scores"]))
    assert np.array_equal(T.bits(hist["valid_scores"]), T.bits(want["valid_scores"]))
    VX, vy, voff = T.dataset(104, rows=600)
    assert np.array_equal(T.bits(booster.predict(VX)), T.bits(hist["valid_scores"]))
    # the last history value of the kept model is the metric of its validation scores
    m = E.mean(E.per_group(E.NDCG, 10, hist["valid_scores"], vy, voff))
    assert T.bits(m) == T.bits(hist["metric"][want["best_iteration"] - 1])
    booster.close()


def test_determinism_and_upload_pieces(ctx, monkeypatch):
    cfg = {"iterations": 3}
    X, y, off = T.dataset(1, rows=3000)
    models = []
    for piece in (None, None, "37"):
        if piece:
            monkeypatch.setenv("MRK_TRAIN_PIECE_ROWS", piece)
        booster, hist = fit_lambdamart(X, y, off, valid=T.dataset(101, rows=500), ctx=ctx, **cfg)
        models.append(hist["model"])
        booster.close()
    assert models[0] == models[1] == models[2] and models[0].count(b"Tree=") == 3


def test_it_learns(ctx):
    """400 groups of 20 rows whose label follows two columns plus noise, 30 iterations; 100 held-out groups.  The restatement's model,
    on the CPU: ndcg@10 0.7974, noop 0.4220, random 0.4076.  The condition is the order of the three, not those numbers."""
    X, y, off = T.learnable(7)
    HX, hy, hoff = T.learnable(8, groups=100)
    booster, hist = fit_lambdamart(X, y, off, ctx=ctx, iterations=30)
    assert hist["best_iteration"] == 30
    res = evaluate(booster, HX, hy, hoff, metrics=(("ndcg", 10),), seed=0)[0]
    print(res)
    assert res["value"] > res["noop"] and res["value"] > res["random"]
    booster.close()
