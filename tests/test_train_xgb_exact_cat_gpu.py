"""GPU: categorical splits under tree_method "exact" (enable_categorical; csrc/train_exact.hip train_exact_cat_sums / _cat_scan and the
categorical form of train_exact_route; include/mrk.h steps 2ec, 5ec) against the histogram grower where the two must agree and against
the restatement (tests/train_xgb_exact_cat_reference.py) everywhere else: models as bytes, scores as bit patterns."""
import json
import os
import re

import numpy as np
import pytest

import train_reference as T
import train_xgb_exact_cat_reference as TXEC
import train_xgb_reference as TX
import metarank_amd as M
from metarank_amd import _native as N
from metarank_amd.train import Trainer, fit_lambdamart

pytestmark = pytest.mark.gpu
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metarank_amd", "csrc")
const = lambda header, name: int(re.search(name + r" = (\d+);", open(os.path.join(CSRC, header)).read()).group(1))
TILE, ROUTES, LDS_MASKS = const("train_exact.hpp", "TRAIN_EXACT_TILE"), const("train_exact.hpp", "TRAIN_EXACT_LDS_ROUTES"), const("train.hpp", "TRAIN_LEVEL_LDS_MASKS")


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def exact(**cfg):
    return dict(cfg, backend="xgboost", tree_method="exact", enable_categorical=True)


def same(hist, want):
    assert hist["model"] == want["model"], (len(hist["model"]), len(want["model"]))
    assert (hist["iterations_run"], hist["best_iteration"]) == (want["iterations_run"], want["best_iteration"])
    assert np.array_equal(T.bits(hist["scores"]), T.bits(want["scores"]))


def mixed(rows, ks, seed=1, nan_share=0.0):
    """T.dataset (column 2: more than 254 distinct cells; 1: NaN) plus an all-NaN column plus one "c" column per entry of ks"""
    X, y, off = T.dataset(seed, rows=rows)
    X, y, ft = TXEC.with_categories(np.column_stack([X, np.full(rows, np.nan)]), y, ks, seed, nan_share)
    return X, y, off, ft


@pytest.mark.parametrize("K", [3, 6, 70])
def test_all_c_exact_is_hist(ctx, K):
    """no rule of a "c" column loses anything to binning and the model text names no method: the same bytes.  K = 3: one against the rest"""
    X, y, off = T.dataset(1, rows=3000)
    X, y, ft = TXEC.with_categories(X[:, :0], y, (K, K, K), seed=K)
    cfg = dict(backend="xgboost", maxDepth=3, iterations=2, sampling=0.5, seed=5, feature_types=ft)
    _, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    _, got = fit_lambdamart(X, y, off, ctx=ctx, **dict(cfg, tree_method="exact", enable_categorical=True))
    trees = json.loads(hist["model"])["learner"]["gradient_booster"]["model"]["trees"]
    assert hist["iterations_run"] == 2 and all(len(t["categories_nodes"]) >= 3 for t in trees)
    assert (K > 3) == any(s > 1 for t in trees for s in t["categories_sizes"])
    same(got, hist)


def hard(nan_wants):
    """300 ids: more than the 253 kept, "other" holds rows; NaN where the labels ask for it; cells no category claims"""
    X, y, off, ft = mixed(3000, (300,), seed=3, nan_share=0.15)
    nan = np.isnan(X[:, 9])
    X[np.flatnonzero(~nan)[:8], 9] = [-1.0, 3.5, 2.0 ** 24, 40000.0] * 2
    return X, np.where(nan, 0.0 if nan_wants == "left" else 4.0, np.clip(y, 1, 3)), off, ft


def wide():
    X, y, off = T.dataset(2, rows=3000)
    X, y, ft = TXEC.with_categories(X[:, [0, 3]], y, (70, 70, 70, 70), seed=2)
    return X, y, off, ft


def unseen():
    VX, vy, voff, _ = mixed(600, (70, 6), seed=102, nan_share=0.02)
    VX[::7, 9] += 1000.0
    return VX, vy, voff


cat_levels = lambda w: np.bincount([t.depth[n] for t in w["trees"][:1] for n in t.cats])
off_bound = lambda w, X: any(t.left[n] >= 0 and n not in t.cats and float(t.cond[n]) not in set(np.float32(TX.bin_bounds(X[:, t.col[n]])).tolist())
                             for t in w["trees"] for n in range(t.num_nodes))
# name -> (data, validation set, config, what the restatement's forest must hold for the case to show anything)
CASES = {
    **{"rows%d" % r: (lambda r=r: mixed(r, (6, 70), seed=7), None, dict(iterations=2, maxDepth=4, min_child_weight=1e-3),   # the root spans every tile, runs straddle them
                      lambda w, X: cat_levels(w).sum() > 0 and off_bound(w, X)) for r in (TILE - 1, TILE + 1, 2 * TILE + 1)},
    **{"nan_" + side: (lambda side=side: hard(side), None, dict(iterations=2, maxDepth=3, sampling=1.0),
                       lambda w, X, side=side: len(w["kept"][9]) == 253 and (w["bins"][9] == 254).sum() > 8 and 0 in w["trees"][0].cats
                       and w["trees"][0].default_left[0] == (side == "left")) for side in ("left", "right")},
    # depth 8 without a weight limit: a level of more categorical nodes than the routing kernel's LDS holds masks, and of more nodes than routes
    "wide": (wide, None, {"iterations": 1, "maxDepth": 8, "sampling": 1.0, "min_child_weight": 0.0, "lambda": 0.01}, lambda w, X: cat_levels(w).max() > max(LDS_MASKS, ROUTES)),
    "valid": (lambda: mixed(1500, (70, 6), seed=2, nan_share=0.02), unseen, dict(iterations=40, early_stopping=3, learningRate=0.3, maxDepth=4),
              lambda w, X: w["best_iteration"] < w["iterations_run"] < 40 and cat_levels(w).sum() > 0),
    "bias": (lambda: mixed(1500, (70,), seed=3), None, dict(iterations=3, maxDepth=4, position_bias={"positions": 8}),
             lambda w, X: w["iterations_run"] == 3 and not np.all(w["t_plus"] == 1.0) and cat_levels(w).sum() > 0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(ctx, name):
    data, valid, cfg, holds = CASES[name]
    X, y, off, ft = data()
    valid, cfg = valid and valid(), exact(feature_types=ft, **cfg)
    want = TXEC.fit(X, y, off, valid=valid, cfg=cfg)
    assert holds(want, X)
    booster, hist = fit_lambdamart(X, y, off, valid=valid, ctx=ctx, **cfg)
    same(hist, want)
    assert np.array_equal(T.bits(booster.predict(X)), T.bits(hist["scores"]))      # the model routes every cell as the trainer did
    if valid:
        assert np.array_equal(T.bits(hist["valid_scores"]), T.bits(want["valid_scores"])) and np.array_equal(T.bits(hist["metric"]), T.bits(want["history"]))
    if "position_bias" in cfg:
        assert np.array_equal(T.bits(hist["position_bias"][0]), T.bits(want["t_plus"]))
    booster.close()


def test_key_rules(ctx):
    X, y, off, ft = mixed(300, (6,))
    xgb = {"backend": "xgboost"}
    cases = [(dict(xgb, tree_method="exact", enable_categorical=1), None, N.ERR_PARSE, ["enable_categorical", "Boolean"]),
             ({"enable_categorical": True}, None, N.ERR_INVALID_ARG, ["enable_categorical is not a key of the lightgbm backend"]),
             (dict(xgb, tree_method="hist", enable_categorical=True), ft, N.ERR_INVALID_ARG, ["enable_categorical", "hist"]),
             (dict(xgb, enable_categorical=True), ft, N.ERR_INVALID_ARG, ["enable_categorical", "hist"]),
             (dict(xgb, tree_method="exact", enable_categorical=False), ft, N.ERR_UNSUPPORTED, ["tree_method", "'c'", "set enable_categorical"])]
    for cfg, types, status, words in cases:
        with pytest.raises(N.MrkError) as e:
            Trainer(cfg, ctx, feature_types=types)
        assert e.value.status == status and all(w in str(e.value) for w in words), str(e.value)
    X[5, 9] = 1e300                                                    # finite, +inf as an f32: refused in a "c" column too
    with pytest.raises(N.MrkError) as e:
        fit_lambdamart(X, y, off, ctx=ctx, **exact(iterations=1, feature_types=ft))
    assert e.value.status == N.ERR_INVALID_ARG and "column 9" in str(e.value) and "row 5" in str(e.value)
    X, y, off = T.dataset(1, rows=TILE + 1)
    plain = dict(xgb, tree_method="exact", iterations=2, maxDepth=4)
    models = [fit_lambdamart(X, y, off, ctx=ctx, **cfg)[1]["model"] for cfg in (plain, dict(plain, enable_categorical=True, feature_types=["q"] * 8))]
    assert models[0] == models[1] and b'"split_type":[0' in models[0]
