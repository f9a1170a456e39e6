"""GPU: categorical splits in the fit of the xgboost backend (feature_types; csrc/train.hip scan_cat_column_xgb and the categorical form of
train_level_split) against their restatement (tests/train_xgb_cat_reference.py): models as bytes, scores as bit patterns, no tolerances.
tests/test_train_xgb_cat_cpu.py asserts on the CPU that every case produces what it is there for."""
import functools

import numpy as np
import pytest

import train_reference as T
import train_xgb_cat_reference as TC
import metarank_amd as M
from metarank_amd import _native as N
from metarank_amd.train import Trainer, fit_lambdamart
from test_train_device_gpu import give

pytestmark = pytest.mark.gpu
want = functools.lru_cache(maxsize=None)(TC.case_fit)


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def device_fit(ctx, name):
    X, y, off, _ = TC.case_data(name)
    return fit_lambdamart(X, y, off, valid=TC.case_valid(name), ctx=ctx, **TC.case_config(name))


@pytest.mark.parametrize("name", list(TC.CASES))
def test_model_bytes(ctx, name):
    hist, r = device_fit(ctx, name)[1], want(name)
    assert (hist["iterations_run"], hist["best_iteration"]) == (r["iterations_run"], r["best_iteration"])
    n = next((i for i, (a, b) in enumerate(zip(hist["model"], r["model"])) if a != b), -1)
    assert hist["model"] == r["model"], (len(hist["model"]), len(r["model"]), n, hist["model"][max(n - 80, 0):n + 40], r["model"][max(n - 80, 0):n + 40])


@pytest.mark.parametrize("name", list(TC.CASES))
def test_scores(ctx, name):
    (booster, hist), r = device_fit(ctx, name), want(name)
    assert np.array_equal(T.bits(hist["scores"]), T.bits(r["scores"]))
    assert np.array_equal(T.bits(booster.predict(TC.case_data(name)[0])), T.bits(hist["scores"]))       # the emitted model, f64 rows in
    if TC.CASES[name][4]:
        assert np.array_equal(T.bits(hist["valid_scores"]), T.bits(r["valid_scores"])) and np.array_equal(T.bits(hist["metric"]), T.bits(r["history"]))
        assert np.array_equal(T.bits(booster.predict(TC.case_valid(name)[0])), T.bits(hist["valid_scores"]))


@pytest.mark.parametrize("name", list(TC.CASES))
def test_special_cells_route_alike(ctx, name):
    """every special cell, every kept id and a few beyond them in every "c" column of a few rows: the loaded model against the restatement"""
    X, _, _, ft = TC.case_data(name)
    rows = []
    for c in np.flatnonzero(np.array(ft) == "c"):
        for v in list(TC.SPECIAL_CELLS) + [-0.5, 0.999, 32764.0, 32765.0, 3e38] + list(np.arange(0.0, 910.0, 1.0 if c == TC.CAT_COLUMNS[0] else 13.0)):
            rows.append(X[len(rows) % 50].copy())
            rows[-1][c] = v
    P = np.array(rows)
    assert np.array_equal(T.bits(device_fit(ctx, name)[0].predict(P)), T.bits(TC.predict(want(name), P)))


@pytest.mark.parametrize("name", ["k70", "valid"])
def test_both_ways_of_handing_over_give_the_same_model(ctx, name):
    X, y, off, _ = TC.case_data(name)
    t = Trainer(TC.case_config(name), ctx)
    give(t, 0, X, y, off, True, pieces=[700, len(y) - 700])
    if TC.case_valid(name):
        give(t, 1, *TC.case_valid(name), True)
    t.fit()
    assert t.model() == device_fit(ctx, name)[1]["model"] and np.array_equal(T.bits(t.scores(0)), T.bits(device_fit(ctx, name)[1]["scores"]))
    t.close()


def test_all_q_is_no_key(ctx):
    X, y, off, ft = TC.case_data("k6")
    cfg = dict(TC.case_config("k6"), feature_types=None)
    models = [fit_lambdamart(X, y, off, ctx=ctx, **dict(cfg, feature_types=f))[1]["model"] for f in (None, ["q"] * len(ft))]
    assert models[0] == models[1] and b'"feature_types":[]' in models[0] and models[0] != device_fit(ctx, "k6")[1]["model"]


def test_the_length_is_checked_against_the_columns(ctx):
    X, y, off, ft = TC.case_data("k3")
    with pytest.raises(N.MrkError) as e:
        fit_lambdamart(X, y, off, ctx=ctx, backend="xgboost", feature_types=ft[:-1])
    assert e.value.status == N.ERR_INVALID_ARG and "7" in e.value.message and "8" in e.value.message
