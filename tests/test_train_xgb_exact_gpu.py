"""GPU: the xgboost backend's fit under tree_method "exact" (csrc/train_exact.hip; include/mrk.h steps 2e, 5e) against its restatement
(tests/train_xgb_exact_reference.py, checked on the CPU in tests/test_train_xgb_exact_cpu.py): models as bytes, scores as bit patterns."""
import json
import os
import re

import numpy as np
import pytest

import train_bias_reference as TB
import train_reference as T
import train_xgb_exact_reference as TXE
import train_xgb_reference as TX
import metarank_amd as M
from metarank_amd import _native as N
from metarank_amd.train import Trainer, bin_bounds, fit_lambdamart

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r"TRAIN_EXACT_TILE = (\d+);", open(os.path.join(REPO, "metarank_amd", "csrc", "train_exact.hpp")).read()).group(1))
ROUTES = int(re.search(r"TRAIN_EXACT_LDS_ROUTES = (\d+);", open(os.path.join(REPO, "metarank_amd", "csrc", "train_exact.hpp")).read()).group(1))


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def exact(**cfg):
    return dict(cfg, backend="xgboost", tree_method="exact")


def same(hist, want):
    assert hist["model"] == want["model"], (len(hist["model"]), len(want["model"]))
    assert (hist["iterations_run"], hist["best_iteration"]) == (want["iterations_run"], want["best_iteration"])
    assert np.array_equal(T.bits(hist["scores"]), T.bits(want["scores"]))


def continuous(rows, seed=1):
    """T.dataset (column 2: more than 254 distinct cells; 1: NaN; 4 and 5: identical; 0: constant) plus a column that is all NaN"""
    X, y, off = T.dataset(seed, rows=rows)
    return np.column_stack([X, np.full(rows, np.nan)]), y, off


def test_exact_is_hist_where_no_bin_holds_two_values(ctx):
    X, y, off = T.dataset(1, rows=3000)
    X = TXE.coarse(X)
    cfg = dict(backend="xgboost", maxDepth=3, iterations=2, sampling=0.5, seed=5)
    _, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    _, got = fit_lambdamart(X, y, off, ctx=ctx, **dict(cfg, tree_method="exact"))
    _, named = fit_lambdamart(X, y, off, ctx=ctx, **dict(cfg, tree_method="hist", max_bin=None))
    assert hist["iterations_run"] == 2 and got["model"] == hist["model"] == named["model"]
    assert np.array_equal(T.bits(got["scores"]), T.bits(hist["scores"]))


@pytest.mark.parametrize("rows", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_row_counts_on_both_sides_of_the_tile(ctx, rows):
    """depth 4: nodes end inside tiles, the root spans all of them (three at 2 x TILE + 1); column 3's runs of equal values straddle tiles"""
    X, y, off = continuous(rows)
    cfg = exact(iterations=2, maxDepth=4, min_child_weight=1e-3)
    want = TXE.fit(X, y, off, cfg=cfg)
    assert want["iterations_run"] == 2 and len(np.unique(X[:, 2].astype(np.float32))) > 254
    assert any(t.col[n] == 2 for t in want["trees"] for n in range(t.num_nodes) if t.left[n] >= 0)
    _, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    same(hist, want)


@pytest.mark.parametrize("cfg", [exact(iterations=2, maxDepth=1, sampling=1.0), exact(iterations=3, maxDepth=3, sampling=0.5, seed=3),
                                 exact(iterations=2, maxDepth=12, sampling=1.0, min_child_weight=0.0), exact(iterations=2, maxDepth=5, gamma=2.0),
                                 exact(iterations=2, maxDepth=5, min_child_weight=20.0)], ids=lambda c: json.dumps(c, sort_keys=True)[:70])
def test_depths_samples_and_admission(ctx, cfg):
    """depth 12 without a weight limit: nodes of one row, and levels of more nodes than the routing kernel's LDS table holds"""
    X, y, off = continuous(3000)
    want = TXE.fit(X, y, off, cfg=cfg)
    assert want["iterations_run"] == cfg["iterations"]
    if cfg["maxDepth"] == 12:
        level = np.bincount([d for t in want["trees"][:1] for d in t.depth])
        assert level.max() > ROUTES and max(want["trees"][0].depth) == 12
    if "gamma" in cfg or cfg.get("min_child_weight", 0) > 1:          # the limit rejects the raw best candidate of some node
        free = TXE.fit(X, y, off, cfg=dict(cfg, gamma=0.0, min_child_weight=1e-3))
        assert free["model"] != want["model"]
    booster, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    same(hist, want)
    assert np.array_equal(T.bits(booster.predict(X)), T.bits(hist["scores"]))      # the model routes every cell as the trainer did
    booster.close()


@pytest.mark.parametrize("nan_wants", ["left", "right"])
def test_nan_on_the_side_the_labels_ask_for(ctx, nan_wants):
    X, y, off = continuous(1500, seed=4)
    nan = np.isnan(X[:, 1])
    y = np.clip(np.where(nan, 0.0 if nan_wants == "left" else 4.0, 1.0 + 2.0 * (X[:, 1] > 0)), 0, 4)
    cfg = exact(iterations=2, maxDepth=2, sampling=1.0)
    want = TXE.fit(X, y, off, cfg=cfg)
    root = want["trees"][0]
    assert root.col[0] == 1 and root.default_left[0] == (1 if nan_wants == "left" else 0)
    _, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    same(hist, want)


def test_validation_and_early_stopping(ctx):
    X, y, off = continuous(1500, seed=2)
    valid = continuous(600, seed=102)
    cfg = exact(iterations=40, early_stopping=3, learningRate=0.3, maxDepth=4)
    want = TXE.fit(X, y, off, valid=valid, cfg=cfg)
    assert want["best_iteration"] < want["iterations_run"] < 40
    _, hist = fit_lambdamart(X, y, off, valid=valid, ctx=ctx, **cfg)
    same(hist, want)
    assert np.array_equal(T.bits(hist["valid_scores"]), T.bits(want["valid_scores"])) and np.array_equal(T.bits(hist["metric"]), T.bits(want["history"]))


def test_position_bias(ctx, monkeypatch):
    X, y, off = continuous(1500, seed=3)
    cfg = exact(iterations=3, maxDepth=4, position_bias={"positions": 8})
    monkeypatch.setattr(TX, "fit", TXE.fit)                            # train_bias_reference wraps the backend's restated fit
    want = TB.fit(X, y, off, cfg=cfg)
    assert want["iterations_run"] == 3 and not np.all(want["t_plus"] == 1.0)
    _, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    same(hist, want)
    assert np.array_equal(T.bits(hist["position_bias"][0]), T.bits(want["t_plus"]))


def test_refusals(ctx):
    X, y, off = T.dataset(1, rows=200)
    cases = [(lambda: Trainer({"backend": "xgboost", "tree_method": "approx"}, ctx), N.ERR_INVALID_ARG, "tree_method = 'approx'"),
             (lambda: Trainer({"tree_method": "exact"}, ctx), N.ERR_INVALID_ARG, "tree_method is not a key of the lightgbm backend"),
             (lambda: Trainer(exact(), ctx, feature_types=["q"] * 7 + ["c"]), N.ERR_UNSUPPORTED, "tree_method"),
             (lambda: bin_bounds(X[:, 2], **exact()), N.ERR_UNSUPPORTED, "tree_method"),
             (lambda: Trainer(exact(), ctx).append_device(0, 256, 10, 8), N.ERR_UNSUPPORTED, "tree_method"),
             (lambda: Trainer(exact(), ctx).seal(0, y, off), N.ERR_UNSUPPORTED, "tree_method")]
    for call, status, words in cases:
        with pytest.raises(N.MrkError) as e:
            call()
        assert e.value.status == status and words in str(e.value), str(e.value)
    X[5, 2] = 1e300                                                    # finite, +inf as an f32: 2x's refusal names column and row
    with pytest.raises(N.MrkError) as e:
        fit_lambdamart(X, y, off, ctx=ctx, **exact(iterations=1))
    assert e.value.status == N.ERR_INVALID_ARG and "column 2" in str(e.value) and "row 5" in str(e.value)
