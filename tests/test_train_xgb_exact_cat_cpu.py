"""CPU: the enable_categorical key in the host half of the library, and the restatement of tree_method "exact" with "c" columns
(tests/train_xgb_exact_cat_reference.py) against the histogram restatement where the two must agree: every column a "c" column."""
import ctypes as C
import json

import numpy as np
import pytest

import train_reference as T
import train_xgb_cat_reference as TXC
import train_xgb_exact_cat_reference as TXEC
from metarank_amd import _native

XGB = {"backend": "xgboost"}
FT = ["q", "c"]


@pytest.mark.parametrize("cfg,status,words", [
    (dict(XGB, tree_method="exact", enable_categorical=True, feature_types=FT), _native.MRK_OK, ()),
    (dict(XGB, tree_method="exact", enable_categorical=True), _native.MRK_OK, ()),
    (dict(XGB, tree_method="exact", enable_categorical=None, feature_types=["q", "q"]), _native.MRK_OK, ()),
    (dict(XGB, tree_method="exact", enable_categorical="true", feature_types=FT), _native.ERR_PARSE, ("enable_categorical", "Boolean")),
    ({"enable_categorical": True}, _native.ERR_INVALID_ARG, ("enable_categorical", "lightgbm")),
    (dict(XGB, tree_method="hist", enable_categorical=True, feature_types=FT), _native.ERR_INVALID_ARG, ("enable_categorical", "hist")),
    (dict(XGB, enable_categorical=False), _native.ERR_INVALID_ARG, ("enable_categorical", "hist")),
    (dict(XGB, tree_method="exact", enable_categorical=False, feature_types=FT), _native.ERR_UNSUPPORTED, ("tree_method", "'c'", "set enable_categorical")),
    (dict(XGB, tree_method="exact", feature_types=FT), _native.ERR_UNSUPPORTED, ("tree_method", "'c'", "set enable_categorical"))],
    ids=lambda v: json.dumps(v)[:60] if isinstance(v, dict) else None)
def test_the_key_in_the_library(cfg, status, words):
    """mrk_train_begin parses the config before it looks at the context: no device"""
    L = _native.lib()
    out = C.c_void_p()
    got = L.mrk_train_begin(None, json.dumps(cfg).encode(), C.byref(out))
    assert got == (status if status != _native.MRK_OK else _native.ERR_INVALID_ARG), cfg   # (a config that parses: the null context is refused next)
    message = L.mrk_last_error().decode()
    assert all(w in message for w in words) and (status != _native.MRK_OK or "null context" in message), message


@pytest.mark.parametrize("K", [3, 6, 70])
def test_all_c_exact_is_hist(K):
    X, y, off = T.dataset(1, rows=3000)
    X, y, ft = TXEC.with_categories(X[:, :0], y, (K, K, K), seed=K)
    cfg = dict(XGB, maxDepth=3, iterations=2, sampling=0.5, seed=5, feature_types=ft)
    hist, got = TXC.fit(X, y, off, cfg=cfg), TXEC.fit(X, y, off, cfg=dict(cfg, tree_method="exact", enable_categorical=True))
    assert hist["iterations_run"] == 2 and all(len(t.cats) >= 3 for t in hist["trees"]) and hist["model"] == got["model"]
    assert np.array_equal(T.bits(hist["scores"]), T.bits(got["scores"]))
