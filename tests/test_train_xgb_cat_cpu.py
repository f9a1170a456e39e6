"""CPU: categorical splits of the xgboost backend (include/mrk.h steps 2cx, 5cx): the rules of the feature_types key, and the
restatement (tests/train_xgb_cat_reference.py) itself - every case of the GPU test produces what it is there for, its model loads with
categorical nodes and the oracle's XGBoost reader predicts its training scores bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import train_reference as T
import train_xgb_cat_reference as TC
from metarank_amd import _native
from oracle.forest import OracleForest
from test_train_xgb_cpu import _begin

case_fit = functools.lru_cache(maxsize=None)(TC.case_fit)


def test_key_rules():
    E_ARG, E_PARSE = _native.ERR_INVALID_ARG, _native.ERR_PARSE
    good = lambda r: r[0] == E_ARG and b"null context" in r[1]                     # a good config, no context
    for ft in (["q", "c"], ["q", "q"], [], None):
        assert good(_begin({"backend": "xgboost", "feature_types": ft})), ft
    st, msg = _begin({"backend": "xgboost", "feature_types": ["q", "float"]})
    assert st == E_ARG and b"float" in msg
    for bad in ("c", {"0": "c"}, 1, ["q", 1], ["q", None], [["c"]]):
        assert _begin({"backend": "xgboost", "feature_types": bad})[0] == E_PARSE, bad
    for cfg in ({"feature_types": ["c"]}, {"backend": "lightgbm", "feature_types": []}):   # a key of the other backend names itself
        st, msg = _begin(cfg)
        assert st == E_ARG and b"feature_types" in msg and b"lightgbm" in msg
    assert good(_begin({"feature_types": None}))
    assert _begin({"backend": "xgboost", "feature_types": ["c"], "categorical": [0]})[0] == _native.ERR_UNSUPPORTED   # pinned: stays refused


@pytest.mark.parametrize("name", list(TC.CASES))
def test_a_case_produces_what_it_is_there_for(name):
    r = case_fit(name)
    assert r["iterations_run"] == TC.CASES[name][5]["iterations"] and TC.CASES[name][0] in TC.purposes(r)
    X, _, _, ft = TC.case_data(name)
    for c in np.flatnonzero(np.array(ft) == "c"):                                  # 2cx: the special cells, and "other" where ids were dropped
        b = TC.bin_column(np.array(TC.SPECIAL_CELLS), r["kept"][c])
        assert list(b[[0, 1, 3, 4]]) == [255, 254, 254, 254] and b[2] == list(r["kept"][c]).index(3)
        assert len(r["kept"][c]) <= 253 and (len(r["kept"][c]) < 253 or (r["bins"][c] == 254).sum() > 10)


@pytest.mark.parametrize("name", ["k3", "k70", "valid"])
def test_the_restatements_model_loads_and_predicts_its_own_scores(name):
    r = case_fit(name)
    info = _native.mrk_model_info()
    assert _native.lib().mrk_model_inspect(1, r["model"], len(r["model"]), C.byref(info)) == _native.MRK_OK
    assert info.n_trees == r["best_iteration"] and info.n_categorical == sum(len(t.cats) for t in r["trees"][:r["best_iteration"]]) > 0
    f = OracleForest.from_xgboost(r["model"])
    assert np.array_equal(T.bits(f.predict(TC.case_data(name)[0])), T.bits(r["scores"]))
    if name == "valid":                                                            # ids the training set never saw go left with "other"
        assert np.array_equal(T.bits(f.predict(TC.case_valid(name)[0])), T.bits(r["valid_scores"]))
