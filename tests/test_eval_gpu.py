"""GPU: the ranking evaluation on the device (csrc/eval.hip through mrk_eval_scores / mrk_model_eval) against the Python
restatement (tests/eval_reference.py): every per-group value and every mean must have its BIT PATTERN, no tolerance.  Group sizes
sit on both sides of every kernel threshold (one wavefront: 64; one workgroup: 4096; beyond: the multi-workgroup sort) and of the
bitonic network's powers of two; group counts on both sides of the four-groups-per-workgroup edge.  Labels under relpow are
integers 0..4 (2^y exact); fractional labels come with relpow off."""
import os

import numpy as np
import pytest

import eval_reference as E
import metarank_amd as M
from metarank_amd import _native as N
from metarank_amd.eval import eval_scores, evaluate, noop_array
from workloads import synth

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8200]
FRACTIONS = np.array([0.0, 0.0, 0.0, 0.5, 1.25, 2.0, 3.7])


@pytest.fixture
def eval_env():
    saved = {k: os.environ.get(k) for k in ("MRK_EVAL_WAVE_MAX", "MRK_EVAL_PIECE_ROWS")}
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def dataset(seed, lens):
    """(scores with ties, integer labels 0..4, fractional labels, offsets)"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = int(off[-1])
    scores = np.round(rng.normal(size=rows), 1)
    ints = rng.integers(0, 5, rows).astype(np.float64) * (rng.random(rows) < 0.4)
    return scores, ints, FRACTIONS[rng.integers(0, len(FRACTIONS), rows)], off


def check(metric, cutoff, scores, labels, off, relpow=True, nolabels=1.0, pis=None):
    """one mrk_eval_scores call against the restatement; returns the device's per-group values"""
    value, groups = eval_scores(scores, labels, off, metric, cutoff, relpow=relpow, nolabels=nolabels, per_group=True)
    want = E.per_group(metric, cutoff, scores, labels, off, relpow, nolabels, pis=pis)
    bad = np.flatnonzero(E.bits(groups) != E.bits(want))
    assert bad.size == 0, (metric, cutoff, relpow, [(int(g), int(off[g + 1] - off[g]), float(groups[g]), float(want[g])) for g in bad[:5]])
    assert E.bits(np.array([value]))[0] == E.bits(np.array([E.mean(want)]))[0]
    return groups


def check_all(scores, ints, fracs, off, cutoffs):
    pis = E.orders(scores, off)
    for k in cutoffs:
        check(E.NDCG, k, scores, ints, off, relpow=True, pis=pis)
        check(E.MAP, k, scores, ints, off, pis=pis)
        check(E.MRR, k, scores, ints, off, pis=pis)
    for k in (0, 10):
        check(E.NDCG, k, scores, fracs, off, relpow=False, nolabels=0.5, pis=pis)
        check(E.MAP, k, scores, fracs, off, relpow=False, pis=pis)


@pytest.mark.parametrize("n", SIZES)
def test_group_size(n):
    scores, ints, fracs, off = dataset(n, [n])
    check_all(scores, ints, fracs, off, sorted({0, 1, 10, n - 1, n, n + 1}))


def test_all_group_sizes_in_one_dataset_shuffled():
    lens = np.random.default_rng(5).permutation(SIZES + [64, 3, 100])
    scores, ints, fracs, off = dataset(99, lens)
    check_all(scores, ints, fracs, off, [0, 1, 10, 64, 4096, 8201])


@pytest.mark.parametrize("n_groups", [1, 3, 4, 5, 5000])
def test_group_counts(n_groups):
    """four groups share a workgroup of the wavefront kernel: 3, 4 and 5 sit around that edge, 5 000 make a grid of 1 250"""
    lens = np.random.default_rng(n_groups).integers(1, 41, n_groups)
    scores, ints, _, off = dataset(1000 + n_groups, lens)
    pis = E.orders(scores, off)
    check(E.NDCG, 10, scores, ints, off, pis=pis)
    check(E.MAP, 5, scores, ints, off, pis=pis)
    check(E.MRR, 0, scores, ints, off, pis=pis)


def special_dataset():
    nan, inf = float("nan"), float("inf")
    rng = np.random.default_rng(7)
    groups = []     # (scores, labels)
    for n in (5, 64, 70, 4100):
        z = np.zeros(n)
        last, first = z.copy(), z.copy()
        last[-1], first[0] = 3.0, 2.0
        mixed = rng.choice(np.array([nan, inf, -inf, 0.0, -0.0, 1.5, -1.5, 1.5]), n)
        lab = rng.integers(0, 5, n).astype(np.float64)
        groups += [(np.full(n, 0.25), lab),                     # all scores equal: the group order stands
                   (np.full(n, nan), lab), (mixed, lab),
                   (np.where(np.arange(n) % 2 == 0, 0.0, -0.0), lab),
                   (np.arange(n, dtype=np.float64), last),      # the only relevant item has the best score ...
                   (-np.arange(n, dtype=np.float64), last),     # ... and the worst: ranked last
                   (rng.normal(size=n), z),                     # no relevant item
                   (rng.normal(size=n), np.full(n, 2.0)),       # all relevant
                   (mixed, first)]
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in groups])]).astype(np.int64)
    return np.concatenate([s for s, _ in groups]), np.concatenate([y for _, y in groups]), off


def test_special_scores_and_label_patterns(eval_env):
    scores, labels, off = special_dataset()
    pis = E.orders(scores, off)
    for wave_max in (None, "0"):
        if wave_max is not None:
            os.environ["MRK_EVAL_WAVE_MAX"] = wave_max
        for k in (0, 1, 10):
            check(E.NDCG, k, scores, labels, off, relpow=True, nolabels=0.125, pis=pis)
            check(E.NDCG, k, scores, labels, off, relpow=False, pis=pis)
            check(E.MAP, k, scores, labels, off, pis=pis)
        mrr = check(E.MRR, 0, scores, labels, off, pis=pis)
    per = 9
    for j, n in enumerate((5, 64, 70, 4100)):
        assert mrr[j * per + 4] == 1.0 and mrr[j * per + 5] == 1.0 / n and mrr[j * per + 6] == 0.0 and mrr[j * per + 7] == 1.0


def test_kernels_agree_to_the_byte(eval_env):
    """MRK_EVAL_WAVE_MAX=0 sends the groups of one wavefront through the workgroup kernel; 17 keeps groups of up to 17"""
    lens = np.random.default_rng(11).integers(1, 65, 300)
    scores, ints, fracs, off = dataset(12, lens)
    got = {}
    for wave_max in ("64", "0", "17"):
        os.environ["MRK_EVAL_WAVE_MAX"] = wave_max
        got[wave_max] = [eval_scores(scores, y, off, m, k, relpow=rp, per_group=True)[1].tobytes()
                         for m, k, y, rp in ((E.NDCG, 10, ints, True), (E.NDCG, 0, fracs, False), (E.MAP, 7, ints, True), (E.MRR, 0, fracs, False))]
    assert got["64"] == got["0"] == got["17"]
    del os.environ["MRK_EVAL_WAVE_MAX"]
    check(E.NDCG, 10, scores, ints, off)


_models = {}


def model_case(kind):
    """(booster, X of about 1 000 rows x 8 columns, integer labels, offsets): built once"""
    if kind not in _models:
        rng = np.random.default_rng(3)
        lens = list(rng.integers(1, 60, 36)) + [150]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        rows = int(off[-1])
        X = rng.normal(size=(rows, 8))
        q = [np.quantile(X[:, j], np.linspace(0.02, 0.98, 49)) for j in range(8)]
        if kind == "lgbm":
            b = M.HipBooster(synth.synthetic_lgbm_model(n_trees=20, n_features=8, quantiles=q, missing="per_feature"), M.LIGHTGBM)
        else:
            b = M.HipBooster(synth.synthetic_xgb_model(n_trees=12, n_features=8, depth=4, quantiles=q), M.XGBOOST)
        labels = rng.integers(0, 5, rows).astype(np.float64) * (rng.random(rows) < 0.3)
        _models[kind] = (b, X, labels, off)
    return _models[kind]


METRICS = [("ndcg", 10), ("map", 5), ("mrr", 0), ("ndcg", 0)]


@pytest.mark.parametrize("kind", ["lgbm", "xgb"])
def test_model_eval(kind, eval_env):
    b, X, labels, off = model_case(kind)
    rows = X.shape[0]
    res, scores = evaluate(b, X, labels, off, METRICS, seed=4, return_scores=True)
    assert scores.tobytes() == b.predictMat(X, rows, X.shape[1]).tobytes()
    assert len(np.unique(scores)) > 10
    rnd = np.random.default_rng(4).random(rows)
    for (name, k), r in zip(METRICS, res):
        m = E.__dict__[name.upper()]
        for what, want in (("value", E.per_group(m, k, scores, labels, off)), ("noop", E.per_group(m, k, None, labels, off, noop=True)),
                           ("random", E.per_group(m, k, rnd, labels, off))):
            assert E.bits(np.array([r[what]]))[0] == E.bits(np.array([E.mean(want)]))[0], (name, k, what, r[what], E.mean(want))
    # noop through the model entry = noopArray fed to the score entry
    for (name, k), r in zip(METRICS, res):
        assert E.bits(np.array([r["noop"]]))[0] == E.bits(np.array([eval_scores(noop_array(off), labels, off, name, k)]))[0]
    # pieces of 37 rows: every group of more than 37 items straddles two, and the scores and values do not move
    os.environ["MRK_EVAL_PIECE_ROWS"] = "37"
    res37, scores37 = evaluate(b, X, labels, off, METRICS, seed=4, return_scores=True)
    os.environ["MRK_EVAL_PIECE_ROWS"] = "1"
    res1 = evaluate(b, X[:70], labels[:70], np.array([0, 30, 70]), METRICS, seed=4)
    del os.environ["MRK_EVAL_PIECE_ROWS"]
    assert scores37.tobytes() == scores.tobytes() and res37 == res
    assert res1 == evaluate(b, X[:70], labels[:70], np.array([0, 30, 70]), METRICS, seed=4)
    # two metrics in one call = two calls
    for i, mk in enumerate(METRICS):
        assert evaluate(b, X, labels, off, [mk], seed=4) == [res[i]]
    # without random scores the third value is NaN; linear gain is another number
    out = np.zeros(3)
    ms, ks = np.array([0], dtype=np.int32), np.array([10], dtype=np.int32)
    N.check(N.lib().mrk_model_eval(b.handle, ms.ctypes.data, ks.ctypes.data, 1, 1, 1.0, X.ctypes.data, 8, labels.ctypes.data, off.ctypes.data, len(off) - 1,
                                   None, out.ctypes.data, None))
    assert out[0] == res[0]["value"] and out[1] == res[0]["noop"] and np.isnan(out[2])
    assert evaluate(b, X, labels, off, [("ndcg", 10)], relpow=False, seed=4)[0]["value"] != res[0]["value"]


def test_model_eval_refusals():
    b, X, labels, off = model_case("xgb")
    with pytest.raises(M.MrkError) as e:
        evaluate(b, np.ascontiguousarray(X[:, :2]), labels, off)
    assert e.value.status == N.ERR_DIM_MISMATCH
    bad = X.copy()
    bad[5, 0] = np.inf
    with pytest.raises(M.MrkError) as p:
        b.predictMat(bad, bad.shape[0], bad.shape[1])
    with pytest.raises(M.MrkError) as e:
        evaluate(b, bad, labels, off)
    assert e.value.status == p.value.status and e.value.message == p.value.message      # as predictMat gives
    assert evaluate(b, X, labels, off)[0]["value"] > 0.0                                 # the flag does not stick
