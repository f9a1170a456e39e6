"""CPU: the restatement of tree_method "exact" (tests/train_xgb_exact_reference.py) - its search against every threshold tried one by one,
its fit against the histogram restatement where no bin holds two values - and the config key in the host half of the library."""
import ctypes as C
import json

import numpy as np
import pytest

import train_reference as T
import train_xgb_exact_reference as TXE
import train_xgb_reference as TX
from metarank_amd import _native

CFG = TX.parse_config({"backend": "xgboost", "min_child_weight": 0.05})


def brute_force(cols32, sample, qg, qh, e_g, e_h, cfg):
    """every (column, bound among the column's values, NaN side) judged on its own in Python floats: (gain, col, bound, nan_left)"""
    lam, gamma, mcw = float(cfg["lambda"]), float(cfg["gamma"]), float(cfg["min_child_weight"])
    real = lambda q, e: float(np.ldexp(float(q), -e))
    term = lambda QG, QH: real(QG, e_g) * real(QG, e_g) / (real(QH, e_h) + lam)
    tg, th = int(qg[sample].sum()), int(qh[sample].sum())
    best = None
    for col, x in enumerate(cols32):
        nan = np.isnan(x)
        for bound in sorted(set(x[~nan].tolist()))[1:]:
            for nan_left in ((0, 1) if (nan & sample).any() else (0,)):
                left = (x < bound) | (nan & bool(nan_left))
                ls, rs = left & sample, ~left & sample
                if not ls.any() or not rs.any():
                    continue
                QGL, QHL = int(qg[ls].sum()), int(qh[ls].sum())
                gain = (term(QGL, QHL) + term(tg - QGL, th - QHL)) - term(tg, th)
                if real(QHL, e_h) >= mcw and real(th - QHL, e_h) >= mcw and gain > gamma and (best is None or gain > best[0]):
                    best = (gain, col, np.float32(bound), nan_left)
    return best


@pytest.mark.parametrize("seed,sampling,extra", [(1, 1.0, {}), (2, 0.5, {}), (3, 1.0, {"min_child_weight": 0.8}), (4, 0.7, {"gamma": 0.02, "lambda": 0.0})])
def test_the_search_against_every_threshold_one_by_one(seed, sampling, extra):
    X, y, off = T.dataset(seed, rows=40)
    X[::7, 2] = np.nan
    cfg = dict(CFG, **extra)
    g, h = T.gradients(np.full(40, 0.5), y.astype(np.int64), [int(o) for o in off])
    e_g, e_h = T.exponent(float(np.abs(g).max()), 40), T.exponent(float(h.max()), 40)
    qg, qh = T.quantise(g, e_g), T.quantise(h, e_h)
    sample = TX.row_sample(40, sampling, 0, seed)
    cols32 = TXE.cells(X)
    got = TXE.best_split(cols32, np.arange(40), sample, qg, qh, e_g, e_h, cfg)
    want = brute_force(cols32, sample, qg, qh, e_g, e_h, cfg)
    assert want is not None and got is not None
    assert (got[0], got[1], got[5], got[3]) == want


@pytest.mark.parametrize("cfg", [{"maxDepth": 2, "iterations": 3, "sampling": 1.0}, {"maxDepth": 3, "iterations": 2, "sampling": 0.5, "seed": 5}])
def test_exact_is_hist_where_no_bin_holds_two_values(cfg):
    """the two searches see the same partitions; they name the same bound as long as every node that splits holds both neighbours of
    the column's values around it - shallow trees over 3 000 rows and 7 values a column"""
    X, y, off = T.dataset(1, rows=3000)
    X = TXE.coarse(X)
    cfg = dict(cfg, backend="xgboost")
    hist, exact = TX.fit(X, y, off, cfg=cfg), TXE.fit(X, y, off, cfg=dict(cfg, tree_method="exact"))
    assert hist["iterations_run"] == cfg["iterations"] and hist["model"] == exact["model"]
    assert np.array_equal(T.bits(hist["scores"]), T.bits(exact["scores"]))
    assert TXE.fit(X, y, off, cfg=dict(cfg, tree_method="hist"))["model"] == hist["model"]


def test_the_key_in_the_library():
    L = _native.lib()
    n = C.c_int(0)
    col = np.arange(4, dtype=np.float64)
    bins = lambda cfg: L.mrk_train_bins(json.dumps(cfg).encode(), col.ctypes.data, 4, None, 0, C.byref(n))
    assert bins({"backend": "xgboost", "tree_method": "hist"}) == _native.MRK_OK and bins({"backend": "xgboost", "tree_method": None}) == _native.MRK_OK
    for cfg, status, words in (({"backend": "xgboost", "tree_method": "approx"}, _native.ERR_INVALID_ARG, ("tree_method", "approx")),
                               ({"tree_method": "exact"}, _native.ERR_INVALID_ARG, ("tree_method", "lightgbm")),
                               ({"backend": "xgboost", "tree_method": "exact"}, _native.ERR_UNSUPPORTED, ("tree_method", "mrk_train_bins")),
                               ({"backend": "xgboost", "tree_method": "exact", "feature_types": ["q", "c"]}, _native.ERR_UNSUPPORTED, ("tree_method", "'c'"))):
        assert bins(cfg) == status, cfg
        message = L.mrk_last_error().decode()
        assert all(w in message for w in words), message
