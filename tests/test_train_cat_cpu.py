"""CPU: categorical columns in the host half of the LambdaMART fit (include/mrk.h steps 2c and 5c): mrk_train_categories against the
restatement (tests/train_cat_reference.py), the new config keys, tests/native/train_cat_host_test.cpp under ASan + UBSan, and the
restatement itself - without a categorical column it gives train_reference's bytes, with two its model text, read by the oracle's
LightGBM reader, predicts its own scores bit for bit, also for cells that have no bin."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import train_cat_reference as TC
import train_reference as T
from metarank_amd import _native
from metarank_amd.train import categorical_columns, kept_categories
from oracle.forest import OracleForest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_logic_native_driver(tmp_path):
    exe = str(tmp_path / "train_cat_host_test")
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(REPO, "tests", "native", "train_cat_host_test.cpp"), os.path.join(csrc, "train_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ALL OK" in out.stdout


def _columns():
    rng = np.random.default_rng(12)
    # 300 ids: id 5 heavy, ids 0 ... 249 three times, ids 250 ... 299 twice: the cut (254 kept) falls among the ids seen twice
    ties = np.concatenate([np.full(500, 5.0), np.repeat(np.arange(250.0), 3), np.repeat(np.arange(250.0, 300.0), 2)])
    return {
        "3 categories": rng.integers(0, 3, 100).astype(np.float64),
        "254 categories": rng.permutation(np.repeat(np.arange(254.0), 3)),
        "300 categories, one heavy, ties at the cut": rng.permutation(ties),
        "NaN, negative, fractional": np.array([2.9, np.nan, -0.5, -1.0, 7.0, -3.5, 2.0, 7.99, np.nan]),
        "only NaN": np.full(20, np.nan),
    }


@pytest.mark.parametrize("name", list(_columns()))
def test_kept_categories_against_the_restatement(name):
    col = _columns()[name]
    want = TC.kept_categories(col)
    got = kept_categories(col)
    assert got.dtype == np.int32 and list(got) == list(want)
    assert list(got) == sorted(set(got))
    if name == "3 categories":
        assert list(got) == [0, 1, 2]
    if name == "254 categories":
        assert list(got) == list(range(254))
    if name.startswith("300"):
        assert list(got) == list(range(254))              # among the ids seen twice the lower ones: 250 ... 253
        assert list(kept_categories(col, max_bin=2)) == [5]
    if name.startswith("NaN"):
        assert list(got) == [0, 2, 7]                     # 2.9 -> 2, -0.5 -> 0, 7.99 -> 7; -1.0 and -3.5 have no category
    if name == "only NaN":
        assert len(got) == 0
    assert list(kept_categories(col, max_bin=3)) == list(TC.kept_categories(col, 3)) and len(kept_categories(col, max_bin=3)) <= 2
    # the bin of every cell, through the table: kept ids in ascending order, everything else 255
    b = TC.bin_cat_column(col, want)
    c = TC.categories(col)
    for i in range(len(col)):
        assert b[i] == (list(want).index(c[i]) if c[i] in want else 255)


def test_kept_categories_refusals():
    for v in (np.inf, -np.inf):
        with pytest.raises(_native.MrkError) as e:
            kept_categories(np.array([1.0, v, 2.0]))
        assert e.value.status == _native.ERR_INVALID_ARG
    with pytest.raises(_native.MrkError) as e:
        kept_categories(np.array([1.0, 32765.0]))
    assert e.value.status == _native.ERR_UNSUPPORTED and "32765" in e.value.message
    assert list(kept_categories(np.array([1.0, 32764.9]))) == [1, 32764]
    with pytest.raises(ValueError):
        TC.kept_categories(np.array([1.0, np.inf]))
    with pytest.raises(OverflowError):
        TC.kept_categories(np.array([1.0, 32765.0]))
    L = _native.lib()
    n = C.c_int(0)
    E = _native.ERR_INVALID_ARG
    assert L.mrk_train_categories(None, None, 0, None, 0, C.byref(n)) == E and L.mrk_train_categories(b"{}", None, 0, None, 0, None) == E
    assert L.mrk_train_categories(b"{}", None, 3, None, 0, C.byref(n)) == E
    assert L.mrk_train_categories(b"{}", None, 0, None, 0, C.byref(n)) == _native.MRK_OK and n.value == 0
    assert L.mrk_abi_version() == 9 and L.mrk_abi_layout(None, 0) == 33   # a new symbol only


def _begin(cfg):
    L = _native.lib()
    out = C.c_void_p()
    text = cfg if isinstance(cfg, bytes) else json.dumps(cfg).encode()
    st = L.mrk_train_begin(None, text, C.byref(out))
    assert not out.value
    return st


# key -> (a good value, values that do not parse as its type, values out of range)
KEYS = {
    "categorical": ([3, 0, 7], [3, "3", [1.5], ["1"], {"a": 1}, [[1]]], [[2, 2], [-1], [0, 5, 0]]),
    "max_cat_to_onehot": (1, ["3", 1.5], [0, -1]),
    "max_cat_threshold": (2, ["3", 2.5], [0]),
    "cat_smooth": (0.5, ["x", [1]], [0, -1.0]),
    "cat_l2": (0.0, ["x"], [-0.1]),
    "min_data_per_group": (1, ["3", 1.5], [0]),
}


def test_every_new_config_key():
    L = _native.lib()
    assert set(KEYS) == set(TC.DEFAULTS) - set(T.DEFAULTS)
    for key, (good, unparsable, out_of_range) in KEYS.items():
        assert _begin({key: good}) == _native.ERR_INVALID_ARG and b"null context" in L.mrk_last_error(), key   # a good config, no context
        assert _begin({key: None}) == _native.ERR_INVALID_ARG and b"null context" in L.mrk_last_error(), key   # the default
        for v in unparsable:
            assert _begin({key: v}) == _native.ERR_PARSE, (key, v)
        for v in out_of_range:
            assert _begin({key: v}) == _native.ERR_INVALID_ARG and key.encode() in L.mrk_last_error(), (key, v)
    assert _begin({"categorical": []}) == _native.ERR_INVALID_ARG and b"null context" in L.mrk_last_error()
    assert _begin({"cat_smoth": 1.0}) == _native.ERR_PARSE and b"unknown key 'cat_smoth'" in L.mrk_last_error()
    with pytest.raises(KeyError):
        TC.parse_config({"cat_smoth": 1.0})
    with pytest.raises(ValueError):
        TC.parse_config({"categorical": [1, 1]})


def test_categorical_columns_of_a_values_layout():
    cols = [("popularity", 0, 1, "single"), ("genre", 1, 1, "category"), ("vec", 2, 4, "vector"), ("referer", 6, 1, "category")]
    assert categorical_columns(cols) == [1, 6] and categorical_columns([]) == []


def test_without_a_categorical_column_the_restatement_is_train_references():
    X, y, off = T.dataset(3, rows=600)
    valid = T.dataset(4, rows=300)
    for cfg in ({"iterations": 3, "min_data_in_leaf": 5}, {"iterations": 3, "sampling": 0.5, "seed": 2, "lambda_l2": 1.0}):
        a, b = T.fit(X, y, off, valid=valid, cfg=cfg), TC.fit(X, y, off, valid=valid, cfg=dict(cfg, categorical=[], cat_l2=3.0))
        assert a["model"] == b["model"] and a["iterations_run"] == b["iterations_run"] == 3
        assert np.array_equal(T.bits(a["scores"]), T.bits(b["scores"])) and np.array_equal(T.bits(a["valid_scores"]), T.bits(b["valid_scores"]))
        assert np.array_equal(T.bits(a["history"]), T.bits(b["history"]))


def test_the_restatements_categorical_model_predicts_its_own_scores():
    """two categorical columns (column 8: ten ids and three rare ones under max_bin = 12, so two ids get no bin - the sorted search;
    column 9: three ids - one-vs-rest); the validation set also holds NaN, a negative id, an id the training set never saw and a rare
    id without a bin: the trainer sends all of them right, and so does the independent reader on the model text"""
    X, y, off = TC.dataset(3, rows=1200)
    VX, vy, voff = TC.dataset(4, rows=400, rare=False)
    VX, odd = TC.odd_cells(VX, 8)
    VX[odd[:8], 9] = [np.nan, -1.0, 5.0, 3.5, np.nan, -2.0, 9.0, 44.0]
    cfg = {"iterations": 5, "min_data_in_leaf": 5, "min_data_per_group": 20, "max_bin": 12, "categorical": [8, 9], "sampling": 1.0, "early_stopping": 5}
    r = TC.fit(X, y, off, valid=(VX, vy, voff), cfg=cfg)
    assert r["iterations_run"] == 5 and r["best_iteration"] >= 1
    assert list(r["kept"][8]) == list(range(10)) + [20] and list(r["kept"][9]) == [0, 1, 2] and r["kept"][0] is None
    assert (TC.bin_cat_column(X[:, 8], r["kept"][8]) == 255).sum() == 3            # ids 21 and 22 of the training set have no bin
    assert set(TC.bin_cat_column(VX[odd, 8], r["kept"][8])) == {255}
    trees = r["trees"][:r["best_iteration"]]
    cat_nodes = [(t.feat[n], t.cat[n]) for t in trees for n in sorted(t.cat)]
    assert {c for c, _ in cat_nodes} == {8, 9}                                      # a node of each mode
    assert any(t.dt[n] != 9 for t in trees for n in range(len(t.dt)))               # and numeric ones
    assert any(sorted(b) == list(TC.MEMBERS) for c, b in cat_nodes if c == 8)       # the set the labels ask for, no interval of ids
    f = OracleForest.from_lightgbm_text(r["model"])
    assert f.n_trees == r["best_iteration"] and f.n_features == 10
    assert np.array_equal(T.bits(f.predict(X)), T.bits(r["scores"]))
    assert np.array_equal(T.bits(f.predict(VX)), T.bits(r["valid_scores"]))
    # all right: a row's prediction does not change when its odd cell becomes another odd cell
    P = VX[odd[:4]].copy()
    Q = P.copy()
    Q[:, 8] = [-7.0, np.nan, 21.0, 1e9]
    assert np.array_equal(T.bits(f.predict(P)), T.bits(f.predict(Q)))
    info = _native.mrk_model_info()
    assert _native.lib().mrk_model_inspect(0, r["model"], len(r["model"]), C.byref(info)) == _native.MRK_OK
    assert info.n_trees == r["best_iteration"] and info.n_features == 10 and info.n_categorical == len(cat_nodes)
    text = r["model"].decode()
    assert "feature_infos=" in text and " 0:1:2:3:4:5:6:7:8:9:20 0:1:2\n" in text
    assert text.count("cat_boundaries=") == sum(1 for t in trees if t.cat) and text.count("num_cat=0\n") == sum(1 for t in trees if not t.cat)
