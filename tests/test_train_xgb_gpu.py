"""GPU: the LambdaMART fit of the xgboost backend (mrk_train_* with backend: "xgboost", csrc/train.hip's level-wise grower) against its
restatement (tests/train_xgb_reference.py): models as bytes, scores as bit patterns, no tolerances.  Every case first asserts on the
restatement's output the property it is there for.  The restatement is checked on the CPU in tests/test_train_xgb_cpu.py."""
import functools
import json
import os
import re

import numpy as np
import pytest

import eval_reference as E
import train_reference as T
import train_xgb_reference as TX
import metarank_amd as M
from metarank_amd.eval import evaluate
from metarank_amd.train import bin_bounds, fit_lambdamart
from oracle.forest import OracleForest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_hpp = open(os.path.join(REPO, "metarank_amd", "csrc", "train.hpp")).read()
HIST_ROWS = int(re.search(r"TRAIN_LEVEL_ROWS = (\d+);", _hpp).group(1))       # rows per workgroup of the level histogram kernel
CHUNK = int(re.search(r"TRAIN_LEVEL_CHUNK = (\d+);", _hpp).group(1))          # built nodes per workgroup of the level histogram kernel
LOW_WEIGHT = 1e-3                                                              # min_child_weight under which 3 000 rows fill their levels


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def first_difference(got: bytes, want: bytes) -> str:
    """the tree and the array of the first byte that differs"""
    n = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    head = want[:n].decode()
    key = re.findall(r'"(\w+)":', head)
    return (f"{len(got)} bytes against {len(want)}; first difference at byte {n}: tree {head.count('tree_param')}, key {key[-1] if key else None}\n"
            f"  device {got[max(n - 60, 0):n + 60]!r}\n  wanted {want[max(n - 60, 0):n + 60]!r}")


def same_model(got: bytes, want: bytes):
    assert got == want, first_difference(got, want)


def same_bits(got, want, what="scores"):
    a, b = T.bits(got), T.bits(want)
    if not np.array_equal(a, b):
        i = int(np.flatnonzero(a != b)[0])
        raise AssertionError(f"{what}: {int((a != b).sum())} of {len(a)} differ, first at row {i}: device {got[i]!r}, wanted {want[i]!r}")


def xgb(**cfg):
    return dict(cfg, backend="xgboost")


@functools.lru_cache(maxsize=None)
def reference_fit(rows, cfg_json, valid_rows=0, seed=1):
    X, y, off = T.dataset(seed, rows=rows)
    valid = T.dataset(100 + seed, rows=valid_rows) if valid_rows else None
    return TX.fit(X, y, off, valid=valid, cfg=json.loads(cfg_json))


def both(ctx, rows, cfg, valid_rows=0, seed=1):
    """(booster, the device's history, the restatement's fit, X); model, scores and counts are compared here"""
    X, y, off = T.dataset(seed, rows=rows)
    valid = T.dataset(100 + seed, rows=valid_rows) if valid_rows else None
    booster, hist = fit_lambdamart(X, y, off, valid=valid, ctx=ctx, **cfg)
    want = reference_fit(rows, json.dumps(cfg, sort_keys=True), valid_rows, seed)
    same_model(hist["model"], want["model"])
    assert hist["iterations_run"] == want["iterations_run"] and hist["best_iteration"] == want["best_iteration"]
    same_bits(hist["scores"], want["scores"])
    if valid_rows:
        same_bits(hist["valid_scores"], want["valid_scores"], "validation scores")
        same_bits(hist["metric"], want["history"], "metric history")
    return booster, hist, want, X


def built_nodes(t, max_depth):
    """per level 1 ... max_depth - 1 how many of its nodes get a histogram of their own: one child of every node that split above"""
    return [sum(1 for n in range(t.num_nodes) if t.depth[n] == d - 1 and t.left[n] >= 0) for d in range(1, max_depth)]


def test_one_split_and_none(ctx):
    X, y, off = T.dataset(2, rows=200)
    X = X[:, [2, 3, 4]]
    cfg = xgb(maxDepth=1, iterations=1, sampling=1.0)
    booster, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    want = TX.fit(X, y, off, cfg=cfg)
    assert want["iterations_run"] == 1 and want["trees"][0].num_nodes == 3
    same_model(hist["model"], want["model"])
    assert hist["iterations_run"] == 1 and hist["best_iteration"] == 1
    same_bits(hist["scores"], want["scores"])
    same_bits(booster.predict(X), hist["scores"], "the booster's prediction")
    booster.close()
    cfg["min_child_weight"] = 1e9
    booster, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    want = TX.fit(X, y, off, cfg=cfg)
    assert booster is None and hist["iterations_run"] == 0 and want["iterations_run"] == 0
    same_model(hist["model"], want["model"])
    assert json.loads(hist["model"])["learner"]["gradient_booster"]["model"]["trees"] == []
    assert (hist["scores"] == 0.5).all() and len(hist["scores"]) == 200


@pytest.mark.parametrize("depth", [3, 4, 6, 8])
def test_depths(ctx, depth):
    cfg = xgb(maxDepth=depth, iterations=5, min_child_weight=LOW_WEIGHT)
    booster, hist, want, X = both(ctx, 3000, cfg)
    trees = want["trees"]
    assert want["iterations_run"] == 5 and all(max(t.depth) == depth for t in trees)
    if depth == 4:
        assert all(t.num_leaves <= 16 for t in trees) and max(t.num_leaves for t in trees) > 8      # the bit-vector scorer's range
    if depth == 8:
        assert max(built_nodes(t, depth)[-1] for t in trees) > CHUNK                                 # its last built level takes several node chunks
        assert max(t.num_leaves for t in trees) > 64
    if depth in (4, 8):
        same_bits(booster.predict(X), hist["scores"], "the booster's prediction")
        same_bits(OracleForest.from_xgboost(hist["model"]).predict(X), hist["scores"], "the oracle's prediction")
        w = booster.weights(X.shape[1])                      # loss_changes is written: Booster.weights() works
        assert w.shape == (X.shape[1],) and w[0] == 0.0 and w.sum() > 0.0    # (column 0 is constant: never split on)
    booster.close()


@pytest.mark.parametrize("rows", [HIST_ROWS - 1, HIST_ROWS, HIST_ROWS + 1, 2 * HIST_ROWS + 1])
def test_row_counts_on_both_sides_of_the_histogram_tile(ctx, rows):
    cfg = xgb(iterations=2, maxDepth=4, min_child_weight=LOW_WEIGHT)
    booster, hist, want, _ = both(ctx, rows, cfg)
    assert want["iterations_run"] == 2 and all(t.num_nodes > 7 for t in want["trees"])
    booster.close()


def test_levels_of_one_node_chunk_one_less_and_one_more(ctx):
    """chosen on the CPU: with min_child_weight 1 and all rows the three trees have levels with CHUNK - 1, CHUNK and CHUNK + 1 built nodes"""
    cfg = xgb(iterations=3, maxDepth=6, min_child_weight=1.0, sampling=1.0)
    booster, hist, want, _ = both(ctx, 3000, cfg)
    counts = {c for t in want["trees"] for c in built_nodes(t, 6)}
    assert {CHUNK - 1, CHUNK, CHUNK + 1} <= counts, counts
    booster.close()


def test_gamma_lambda_and_min_child_weight_each_change_the_forest(ctx):
    base = xgb(iterations=3, maxDepth=5)
    models = {}
    for name, extra in (("base", {}), ("gamma", {"gamma": 2.0}), ("lambda", {"lambda": 50.0}), ("lambda 0", {"lambda": 0.0}), ("min_child_weight", {"min_child_weight": 20.0})):
        booster, hist, want, _ = both(ctx, 3000, dict(base, **extra))
        assert want["iterations_run"] == 3
        models[name] = want["model"]
        booster.close()
    assert len(set(models.values())) == len(models)
    nodes = lambda m: sum(int(t["tree_param"]["num_nodes"]) for t in json.loads(m)["learner"]["gradient_booster"]["model"]["trees"])
    assert nodes(models["gamma"]) < nodes(models["base"]) and nodes(models["min_child_weight"]) < nodes(models["base"])   # both prune


def test_cells_at_a_bound_and_one_f32_ulp_beside_it(ctx):
    """TX.adjacent: column 3 holds prev32(1), 1, next32(1), 2 and f64 cells 1 +- 1e-12 that are exactly 1.0f; the labels ask for the
    bound at next32(1).  f64-side binning would put 1 + 1e-12 right of a bound at 1 + ulp32 / 2 and 1 - 1e-12 left of a bound at 1."""
    X, y, off = TX.adjacent(3)
    above = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    col = X[:, 3]
    assert ((col != 1.0) & (col.astype(np.float32) == np.float32(1.0))).sum() > 50
    bounds = TX.bin_bounds(col)
    assert list(bounds) == [1.0, above, 2.0]
    assert np.array_equal(T.bits(bin_bounds(col, backend="xgboost")), T.bits(bounds))
    cfg = xgb(iterations=4, min_child_weight=LOW_WEIGHT, sampling=1.0, maxDepth=4)
    booster, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    want = TX.fit(X, y, off, cfg=cfg)
    found = {float(t.cond[n]) for t in want["trees"] for n in range(t.num_nodes) if t.left[n] >= 0 and t.col[n] == 3}
    assert above in found or 1.0 in found, found
    same_model(hist["model"], want["model"])
    same_bits(hist["scores"], want["scores"])                       # the bin kernel routed every cell as the restatement's f32 bins
    same_bits(booster.predict(X), hist["scores"], "the booster's prediction")
    same_bits(OracleForest.from_xgboost(hist["model"]).predict(X), hist["scores"], "the oracle's prediction")
    booster.close()


def test_row_sampling(ctx):
    models = []
    for cfg in (xgb(iterations=3, maxDepth=4, sampling=0.5, seed=3), xgb(iterations=3, maxDepth=4, sampling=0.5, seed=4), xgb(iterations=3, maxDepth=4, sampling=1.0, seed=3)):
        booster, hist, want, X = both(ctx, 3000, cfg)
        assert want["iterations_run"] == 3
        inside = np.mean([s.mean() for s in want["samples"]])
        assert inside == 1.0 if cfg["sampling"] == 1.0 else 0.45 < inside < 0.55
        if cfg["sampling"] < 1.0:                                   # a row outside every tree's sample is still scored as the model predicts it
            never = ~np.any(want["samples"], axis=0)
            assert never.sum() > 100
            same_bits(booster.predict(X)[never], hist["scores"][never], "unsampled rows")
        same_bits(booster.predict(X), hist["scores"], "the booster's prediction")
        models.append(want["model"])
        booster.close()
    assert len(set(models)) == 3


def test_early_stopping(ctx):
    """seed 2, chosen on the CPU: with early_stopping = 3 the restatement stops after 6 of 40 iterations and keeps 3"""
    cfg = xgb(iterations=40, early_stopping=3, learningRate=0.3, maxDepth=4)
    booster, hist, want, X = both(ctx, 1500, cfg, valid_rows=600, seed=2)
    assert want["iterations_run"] < 40 and want["best_iteration"] < want["iterations_run"]
    assert len(json.loads(hist["model"])["learner"]["gradient_booster"]["model"]["trees"]) == want["best_iteration"]
    VX, vy, voff = T.dataset(102, rows=600)
    same_bits(booster.predict(VX), hist["valid_scores"], "the booster's prediction of the validation rows")
    m = E.mean(E.per_group(E.NDCG, 10, hist["valid_scores"], vy, voff))
    assert T.bits(m) == T.bits(hist["metric"][want["best_iteration"] - 1])
    booster.close()


def test_determinism_and_upload_pieces(ctx, monkeypatch):
    cfg = xgb(iterations=3, maxDepth=6)
    X, y, off = T.dataset(1, rows=3000)
    models = []
    for piece in (None, None, "37"):
        if piece:
            monkeypatch.setenv("MRK_TRAIN_PIECE_ROWS", piece)
        booster, hist = fit_lambdamart(X, y, off, valid=T.dataset(101, rows=500), ctx=ctx, **cfg)
        models.append(hist["model"] + hist["scores"].tobytes() + hist["valid_scores"].tobytes())
        booster.close()
    assert models[0] == models[1] == models[2] and models[0].count(b"tree_param") == 3


def test_it_learns(ctx):
    """400 groups of 20 rows whose label follows two columns plus noise, 30 iterations of the default config; 100 held-out groups.  The
    restatement's model, on the CPU: ndcg@10 0.7961, noop 0.4220, random 0.4076.  The condition is the order of the three."""
    X, y, off = T.learnable(7)
    HX, hy, hoff = T.learnable(8, groups=100)
    booster, hist = fit_lambdamart(X, y, off, ctx=ctx, backend="xgboost", iterations=30)
    assert hist["best_iteration"] == 30
    res = evaluate(booster, HX, hy, hoff, metrics=(("ndcg", 10),), seed=0)[0]
    print(res)
    assert res["value"] > res["noop"] and res["value"] > res["random"]
    booster.close()


def test_the_default_backend_is_untouched(ctx):
    X, y, off = T.dataset(1, rows=3000)
    cfg = {"numLeaves": 16, "iterations": 5}
    want = T.fit(X, y, off, cfg=cfg)
    for extra in ({}, {"backend": "lightgbm"}):
        booster, hist = fit_lambdamart(X, y, off, ctx=ctx, **dict(cfg, **extra))
        assert hist["model"] == want["model"] and want["iterations_run"] == 5
        same_bits(hist["scores"], want["scores"])
        booster.close()
