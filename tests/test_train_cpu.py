"""CPU: the host half of the LambdaMART fit (csrc/train_host.cpp; tests/native/train_host_test.cpp under ASan + UBSan), everything of
mrk_train_* that needs no device (the config decoder, the bins, the argument checks), and the Python restatement the GPU tests
compare with (tests/train_reference.py): its model text, read by the oracle's LightGBM reader, predicts its own training scores bit
for bit."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import train_reference as T
from metarank_amd import _native
from metarank_amd.train import bin_bounds
from oracle.forest import OracleForest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_logic_native_driver(tmp_path):
    exe = str(tmp_path / "train_host_test")
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(REPO, "tests", "native", "train_host_test.cpp"), os.path.join(csrc, "train_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ALL OK" in out.stdout
    # the library's feature-subset sequences are the restatement's: three seeds (one negative) x four trees x four shapes
    lines = re.findall(r"subset cols=(\d+) sampling=(\S+) seed=(-?\d+) tree=(\d+):([ 0-9]*)", out.stdout)
    assert len(lines) == 48 and {int(s) for _, _, s, _, _ in lines} == {0, 12345, -7}
    for cols, sampling, seed, tree, got in lines:
        assert [int(x) for x in got.split()] == T.feature_subset(int(cols), float(sampling), int(seed), int(tree)), (cols, sampling, seed, tree)


def _columns():
    rng = np.random.default_rng(11)
    x = 0.3
    heavy = rng.integers(0, 1000, 5000).astype(np.float64)
    heavy[:1000] = np.arange(1000)                       # all 1 000 values occur
    heavy[rng.permutation(5000)[:3000]] = 417.0          # one value holds (at least) 60 % of the cells
    return {
        "constant": np.full(50, 2.5),
        "3 distinct": rng.integers(0, 3, 100).astype(np.float64),
        "254 distinct": rng.permutation(np.repeat(np.arange(254.0), 3)),
        "255 distinct": rng.permutation(np.repeat(np.arange(255.0), 3)),
        "1000 distinct, one heavy": heavy,
        "neighbours": np.array([x, np.nextafter(x, 1.0)] * 4 + [np.nextafter(x, 0.0)]),
        "zeros": np.array([-0.0, 0.0, -0.0, 1.0, -1.0]),
        "30 % NaN": np.where(rng.random(1000) < 0.3, np.nan, rng.normal(size=1000)),
        "all NaN": np.full(20, np.nan),
    }


@pytest.mark.parametrize("name", list(_columns()))
def test_bins_against_the_restatement(name):
    col = _columns()[name]
    want = T.bin_bounds(col)
    got = bin_bounds(col)
    assert np.array_equal(T.bits(got), T.bits(want)), (len(got), len(want))
    d = len(np.unique(col[~np.isnan(col)] + 0.0))
    assert len(got) == (max(d - 1, 0) if d <= 254 else len(want))
    assert len(got) <= 253 and (np.diff(got) > 0).all()
    if name == "254 distinct":
        assert len(got) == 253                            # every value its own bin
    if name == "255 distinct":
        assert len(got) <= 253                            # one more value: the walk over quantiles
    if name == "neighbours":
        assert len(got) == 2 and set(got) <= set(col)     # no f64 lies between the values: the lower one is the bound
    if name == "zeros":
        assert list(got) == [-0.5, 0.5]
    # bin(x) agrees with the scorer's x <= threshold -> left on every cell and on the neighbours of every bound
    probe = np.concatenate([col, got, np.nextafter(got, np.inf), np.nextafter(got, -np.inf)])
    b = T.bin_column(probe, got)
    for i, v in enumerate(probe):
        assert b[i] == (255 if v != v else int(np.sum(got < v)))
    # another max_bin
    assert np.array_equal(T.bits(bin_bounds(col, max_bin=16)), T.bits(T.bin_bounds(col, 16)))
    assert len(bin_bounds(col, max_bin=16)) <= 14


def test_bins_refuse_an_infinite_cell():
    for v in (np.inf, -np.inf):
        with pytest.raises(_native.MrkError) as e:
            bin_bounds(np.array([1.0, v, 2.0]))
        assert e.value.status == _native.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        T.bin_bounds(np.array([1.0, np.inf]))


def _begin(cfg):
    L = _native.lib()
    out = C.c_void_p()
    text = cfg if isinstance(cfg, bytes) else json.dumps(cfg).encode()
    st = L.mrk_train_begin(None, text, C.byref(out))
    assert not out.value
    return st


# key -> (a good value, values that do not parse as its type, values out of range)
KEYS = {
    "iterations": (7, ["3", 1.5, True], [0, -1]),
    "learningRate": (0.3, ["x", [1]], [0, -0.1]),
    "ndcgCutoff": (5, ["3", 2.5], [0]),
    "maxDepth": (3, ["3", 0.5], [0]),
    "seed": (-4, ["3", 1.5, 2 ** 31], []),
    "numLeaves": (31, ["3", 3.5], [1, 0]),
    "sampling": (0.5, ["x"], [0, 1.5, -1]),
    "debias": (False, [1, "true"], []),
    "max_bin": (16, ["3", 7.5], [1, 256]),
    "truncation": (10, ["3", 1.5], [0]),
    "sigma": (2.0, ["x"], [0, -1]),
    "min_data_in_leaf": (1, ["3", 1.5], [0]),
    "min_sum_hessian": (0.0, ["x"], [-1]),
    "lambda_l2": (1.0, ["x"], [-1]),
    "early_stopping": (3, ["3", 1.5], [0]),
}


def test_every_config_key():
    L = _native.lib()
    assert set(KEYS) == set(T.DEFAULTS)
    for key, (good, unparsable, out_of_range) in KEYS.items():
        assert _begin({key: good}) == _native.ERR_INVALID_ARG and b"null context" in L.mrk_last_error(), key   # a good config, no context
        assert _begin({key: None}) == _native.ERR_INVALID_ARG and b"null context" in L.mrk_last_error(), key   # Option: the default
        for v in unparsable:
            assert _begin({key: v}) == _native.ERR_PARSE, (key, v)
        for v in out_of_range:
            assert _begin({key: v}) == _native.ERR_INVALID_ARG and key.encode() in L.mrk_last_error(), (key, v)
    assert _begin(b'{"iterations":3') == _native.ERR_PARSE
    assert _begin(b"[1]") == _native.ERR_PARSE
    assert _begin({"num_leaves": 16}) == _native.ERR_PARSE and b"unknown key 'num_leaves'" in L.mrk_last_error()
    assert _begin({"debias": True}) == _native.ERR_UNSUPPORTED
    assert _begin({"numLeaves": 4097}) == _native.ERR_UNSUPPORTED and b"4097" in L.mrk_last_error()
    with pytest.raises(KeyError):
        T.parse_config({"num_leaves": 16})


def test_null_arguments_and_argument_checks_without_a_device():
    L = _native.lib()
    E = _native.ERR_INVALID_ARG
    out = C.c_void_p()
    n = C.c_int(0)
    need = C.c_size_t(0)
    assert L.mrk_train_begin(None, None, C.byref(out)) == E and L.mrk_train_begin(None, b"{}", None) == E
    assert L.mrk_train_set(None, 0, None, 1, 1, None, None, 1) == E and L.mrk_train_fit(None) == E
    assert L.mrk_train_model(None, None, 0, C.byref(need)) == E and L.mrk_train_history(None, None, None, None, 0) == E
    assert L.mrk_train_scores(None, 0, None) == E
    L.mrk_train_free(None)
    assert L.mrk_train_bins(None, None, 0, None, 0, C.byref(n)) == E and L.mrk_train_bins(b"{}", None, 0, None, 0, None) == E
    assert L.mrk_train_bins(b"{}", None, 3, None, 0, C.byref(n)) == E
    assert L.mrk_train_bins(b"{}", None, 0, None, 0, C.byref(n)) == _native.MRK_OK and n.value == 0
    assert L.mrk_train_bins(b'{"max_bin":1}', None, 0, None, 0, C.byref(n)) == E

    def grads(scores, labels, offsets, cfg=b"{}"):
        s, y, off = np.asarray(scores, dtype=np.float64), np.asarray(labels, dtype=np.float64), np.asarray(offsets, dtype=np.int64)
        g, h = np.zeros(len(s) + 1), np.zeros(len(s) + 1)
        return L.mrk_train_gradients(None, cfg, s.ctypes.data, y.ctypes.data, off.ctypes.data, len(off) - 1, g.ctypes.data, h.ctypes.data)

    # everything is judged before the context: a good call fails on the null context alone
    assert grads([0.0, 1.0], [0, 1], [0, 2]) == E and b"null context" in L.mrk_last_error()
    assert grads([0.0, 1.0], [0, 1], [1, 2]) == E and b"start at 0" in L.mrk_last_error()
    assert grads([0.0, 1.0], [0, 1], [0, 2, 2]) == E and b"empty" in L.mrk_last_error()
    assert grads([0.0, 1.0], [0, 1], [0, 2, 1]) == E
    assert grads([0.0, 1.0], [0, 0.5], [0, 2]) == E and b"label 1" in L.mrk_last_error()
    assert grads([0.0, 1.0], [31, 0], [0, 2]) == E and b"label 0" in L.mrk_last_error()
    assert grads([0.0, 1.0], [-1, 0], [0, 2]) == E
    assert grads([0.0, 1.0], [np.nan, 0], [0, 2]) == E
    assert grads([0.0, np.inf], [0, 1], [0, 2]) == E and b"score 1" in L.mrk_last_error()
    assert grads([0.0, 1.0], [30, 0], [0, 2]) == E and b"null context" in L.mrk_last_error()
    assert grads(np.zeros(4097), np.zeros(4097), [0, 4097]) == _native.ERR_UNSUPPORTED and b"4097" in L.mrk_last_error()
    assert grads([0.0], [0], [0, 1], b'{"sigma":0}') == E
    assert L.mrk_train_gradients(None, b"{}", None, None, None, 1, None, None) == E
    assert L.mrk_abi_version() == 9 and L.mrk_abi_layout(None, 0) == 33   # new symbols only


def test_feature_subsets_for_three_seeds():
    for seed in (0, 1, 2 ** 31 - 1):
        seen = set()
        for tree in range(20):
            s = T.feature_subset(24, 0.8, seed, tree)
            assert len(s) == 19 and s == sorted(set(s)) and 0 <= s[0] and s[-1] < 24
            seen.add(tuple(s))
        assert len(seen) > 10
    assert T.feature_subset(24, 0.8, 0, 0) != T.feature_subset(24, 0.8, 1, 0)
    assert T.feature_subset(8, 1.0, 5, 3) == list(range(8)) and len(T.feature_subset(3, 0.1, 0, 0)) == 1
    assert len(T.feature_subset(5, 0.5, 0, 0)) == 3                       # floor(2.5 + 0.5)
    assert T.feature_subset(24, 0.8, -1, 2) == T.feature_subset(24, 0.8, 2 ** 32 - 1, 2)   # the seed is taken as its 32 bits


def test_the_restatements_model_predicts_its_own_scores():
    """pins the writer and LightGBM's numbering on a data set with a NaN column; after a first fit cells are moved next to the
    thresholds its trees use, which moves the bounds too: where they land is chance here, and
    test_cells_at_a_bound_and_one_ulp_beside_it has the construction that puts cells at a bound"""
    X, y, off = T.dataset(3, rows=1200)
    cfg = {"iterations": 4, "min_data_in_leaf": 5}
    first = T.fit(X, y, off, cfg=cfg)
    thr = sorted({(t.feat[n], t.thr[n]) for t in first["trees"] for n in range(len(t.feat))})
    assert len(thr) > 10
    rng = np.random.default_rng(0)
    for col, v in thr:
        if col in (2, 4, 6, 7):                                # (the continuous columns; 4's copy 5 is left alone: the copies part)
            i = rng.integers(0, len(X), 3)
            X[i[0], col], X[i[1], col], X[i[2], col] = v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)
    r = T.fit(X, y, off, cfg=cfg)
    assert r["iterations_run"] == 4 and r["best_iteration"] == 4
    f = OracleForest.from_lightgbm_text(r["model"])
    assert f.n_trees == 4 and f.n_features == 8
    assert np.array_equal(T.bits(f.predict(X)), T.bits(r["scores"]))
    assert any((t.dt[n] & 2) for t in r["trees"] for n in range(len(t.dt))) or any(t.feat[n] == 1 for t in r["trees"] for n in range(len(t.feat)))
    # the library's own reader takes the text too (mrk_model_inspect: host only)
    info = _native.mrk_model_info()
    assert _native.lib().mrk_model_inspect(0, r["model"], len(r["model"]), C.byref(info)) == _native.MRK_OK
    assert info.n_trees == 4 and info.n_features == 8
    # a validation set: the history is the metric of the validation scores, the model stops at the best iteration
    VX, vy, voff = T.dataset(4, rows=400)
    rv = T.fit(X, y, off, valid=(VX, vy, voff), cfg=dict(cfg, iterations=12, early_stopping=2, learningRate=0.5))
    assert len(rv["history"]) == rv["iterations_run"] and rv["best_iteration"] == int(np.argmax(rv["history"])) + 1
    fv = OracleForest.from_lightgbm_text(rv["model"])
    assert fv.n_trees == rv["best_iteration"]
    assert np.array_equal(T.bits(fv.predict(VX)), T.bits(rv["valid_scores"])) and np.array_equal(T.bits(fv.predict(X)), T.bits(rv["scores"]))


def test_cells_at_a_bound_and_one_ulp_beside_it():
    """the agreement of bin(x) = #(bounds < x) with the scorer's x <= threshold -> left, on cells that ARE a threshold of the final
    model and on their neighbours one ulp either side (T.adjacent builds the column; nothing here is chance)"""
    X, y, off = T.adjacent(3)
    lo, hi = np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)
    b = T.bin_bounds(X[:, 3])
    assert list(b[:2]) == [lo, 1.0] and len(b) == 3          # no f64 lies between the neighbours: the lower one is the bound
    assert list(bin_bounds(X[:, 3])) == list(b)
    assert list(T.bin_column(np.array([lo, 1.0, hi, 2.0]), b)) == [0, 1, 2, 3]
    r = T.fit(X, y, off, cfg={"iterations": 4, "min_data_in_leaf": 5})
    thr = {t.thr[n] for t in r["trees"] for n in range(len(t.feat)) if t.feat[n] == 3}
    assert 1.0 in thr                                        # the split the labels ask for is AT the value 1.0
    for v in (lo, 1.0, hi):                                  # cells at the threshold and one ulp on either side
        assert (X[:, 3] == v).sum() > 50
    f = OracleForest.from_lightgbm_text(r["model"])
    assert np.array_equal(T.bits(f.predict(X)), T.bits(r["scores"]))
    # a wrong side for one of them would show: the two sides of that split predict differently
    t = next(t for t in r["trees"] if 1.0 in [t.thr[n] for n in range(len(t.feat)) if t.feat[n] == 3])
    P = X[:1].repeat(2, axis=0)
    P[0, 3], P[1, 3] = 1.0, hi
    assert f.predict(P)[0] != f.predict(P)[1]


def test_ties_go_to_the_lowest_bin_before_nan_right():
    """the stated order: the highest gain, then the lowest column, then the lowest bin, then NaN to the right.  A histogram whose bins
    0 and 2 hold the same sums: (b = 0, NaN left) and (b = 1, NaN right) cut the leaf into the same two halves, swapped, so their gains
    are the same f64; the counts admit neither (b = 0, NaN right) nor (b = 1, NaN left).  The lower bin wins, although it sends NaN left."""
    G, H, C = (np.zeros((1, 256), dtype=np.int64) for _ in range(3))
    for b, (g, h, c) in {0: (-400, 300, 5), 1: (900, 700, 30), 2: (-400, 300, 5), 255: (250, 500, 20)}.items():
        G[0, b], H[0, b], C[0, b] = g << 20, h << 20, c
    cfg = T.parse_config({"min_data_in_leaf": 20, "min_sum_hessian": 0.0})
    gain, col, b, nan_left, left = T._best_split((G, H, C), [0], [3], 20, 20, cfg)
    assert (col, b, nan_left) == (0, 0, 1) and left == ((-400 + 250) << 20, (300 + 500) << 20, 25) and gain > 0
    # the same histogram in a second column: the lower column wins the tie between columns
    G2, H2, C2 = (np.concatenate([a, a]) for a in (G, H, C))
    assert T._best_split((G2, H2, C2), [4, 9], {4: 3, 9: 3}, 20, 20, cfg)[1:4] == (4, 0, 1)
