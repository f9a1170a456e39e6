"""GPU: categorical columns in the LambdaMART fit (include/mrk.h steps 2c and 5c; csrc/train.hip: the binning through id -> bin
tables, scan_cat_column, train_split_cat_kernel, the categorical validation walk) against the restatement
(tests/train_cat_reference.py): model bytes, history and scores bit for bit, no tolerances, and HipBooster.predict of every model
against the trainer's own scores.  The restatement is checked against the oracle's reader in tests/test_train_cat_cpu.py."""
import numpy as np
import pytest

import eval_reference as E
import train_cat_reference as TC
import train_reference as T
import metarank_amd as M
from metarank_amd import _native
from metarank_amd.eval import evaluate
from metarank_amd.train import categorical_columns, fit_lambdamart
from oracle.forest import OracleForest

pytestmark = pytest.mark.gpu

SMALL = {"iterations": 2, "min_data_in_leaf": 5, "min_data_per_group": 5, "cat_smooth": 1.0, "sampling": 1.0, "categorical": [1]}


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def first_difference(got: bytes, want: bytes) -> str:
    tree = None
    gl, wl = got.decode().split("\n"), want.decode().split("\n")
    for i, (a, b) in enumerate(zip(gl, wl)):
        if a.startswith("Tree="):
            tree = a
        if a != b:
            return f"{tree}, line {i}:\n  device {a[:300]}\n  wanted {b[:300]}"
    return f"{len(gl)} lines against {len(wl)}"


def both(ctx, X, y, off, cfg, valid=None):
    """the device's fit and the restatement's: the same bytes, history and scores; the scorer predicts the trainer's scores"""
    booster, hist = fit_lambdamart(X, y, off, valid=valid, ctx=ctx, **cfg)
    want = TC.fit(X, y, off, valid=valid, cfg=cfg)
    assert hist["model"] == want["model"], first_difference(hist["model"], want["model"])
    assert hist["iterations_run"] == want["iterations_run"] and hist["best_iteration"] == want["best_iteration"]
    assert np.array_equal(T.bits(hist["scores"]), T.bits(want["scores"]))
    if valid is not None:
        assert np.array_equal(T.bits(hist["metric"]), T.bits(want["history"]))
        assert np.array_equal(T.bits(hist["valid_scores"]), T.bits(want["valid_scores"]))
    if booster is not None:
        assert np.array_equal(T.bits(booster.predict(X)), T.bits(hist["scores"]))
        if valid is not None:
            assert np.array_equal(T.bits(booster.predict(valid[0])), T.bits(hist["valid_scores"]))
    else:
        assert want["best_iteration"] == 0
    return booster, hist, want


def offsets(rng, rows, lo=5, hi=40):
    sizes = []
    while sum(sizes) < rows:
        sizes.append(int(rng.integers(lo, hi + 1)))
    sizes[-1] -= sum(sizes) - rows
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def two_columns(seed, ids, counts, base, nan=0):
    """column 0 noise, column 1 categorical: counts[k] cells of ids[k] and `nan` NaN cells, shuffled; the label is base[k] plus noise
    (1 for a NaN cell), so the category carries the signal"""
    rng = np.random.default_rng(seed)
    k = rng.permutation(np.repeat(np.arange(len(ids) + 1), list(counts) + [nan]))
    rows = len(k)
    cat = np.append(np.asarray(ids, dtype=np.float64), np.nan)[k]
    y = np.clip(np.rint(np.append(np.asarray(base, dtype=np.float64), 1.0)[k] + rng.normal(size=rows) * 0.4), 0, 4)
    return np.column_stack([rng.normal(size=rows), cat]), y, offsets(rng, rows)


def cat_nodes(want, col=None):
    return [(t.feat[n], t.cat[n]) for t in want["trees"] for n in sorted(t.cat) if col is None or t.feat[n] == col]


def root_search(X, y, off, col, cfg):
    """the restatement's categorical search of column `col` on the root histogram of the first iteration:
    (best candidate, [(key, bin)] of the eligible bins in order)"""
    c = TC.parse_config(cfg)
    rows = len(y)
    g, h = T.gradients(np.zeros(rows), y, [int(o) for o in off], float(c["sigma"]), int(c["truncation"]))
    e_g, e_h = T.exponent(float(np.max(np.abs(g))), rows), T.exponent(float(np.max(h)), rows)
    kept = TC.kept_categories(X[:, col], int(c["max_bin"]))
    G, H, C = T._histogram([TC.bin_cat_column(X[:, col], kept)], [0], np.arange(rows), T.quantise(g, e_g), T.quantise(h, e_h))
    return TC.best_cat_split(G[0], H[0], C[0], len(kept), col, e_g, e_h, c), TC.cat_keys(G[0], H[0], C[0], len(kept), e_g, e_h, c)


# ------------------------------------------------------------------ modes and edges of the scan
@pytest.mark.parametrize("K", [1, 2, 4, 5])
def test_k_on_both_sides_of_max_cat_to_onehot(ctx, K):
    """K <= 4: one bin against the rest (K = 1: against the NaN cells alone); K = 5: the sorted search"""
    base = [3, 0, 3, 1, 0][:K]
    X, y, off = two_columns(20 + K, list(range(K)), [120] * K, base, nan=90)
    booster, hist, want = both(ctx, X, y, off, SMALL)
    assert want["nbins"][1] == K and want["iterations_run"] == 2
    nodes = cat_nodes(want, 1)
    assert nodes and (K == 5 or all(len(b) == 1 for _, b in nodes))
    if K == 5:
        assert any(len(b) > 1 for _, b in nodes)
    booster.close()


@pytest.mark.parametrize("m, cat_smooth", [(0, 400.0), (1, 250.0), (2, 150.0), (3, 50.0)])
def test_eligible_bins_0_to_3(ctx, m, cat_smooth):
    """five categories of 300, 200, 100, 20 and 10 cells: cat_smooth decides how many are eligible at the root, and
    max_num = (m + 1) / 2 is 0, 1, 1 and 2"""
    counts = [300, 200, 100, 20, 10]
    X, y, off = two_columns(31, [0, 1, 2, 3, 4], counts, [3, 0, 3, 1, 0])
    cfg = dict(SMALL, cat_smooth=cat_smooth)
    best, keys = root_search(X, y, off, 1, cfg)
    assert len(keys) == m == sum(c >= cat_smooth for c in counts)
    booster, hist, want = both(ctx, X, y, off, cfg)
    assert want["iterations_run"] == 2
    nodes = cat_nodes(want, 1)
    if m == 0:
        assert best is None and not nodes
    else:
        assert best is not None and nodes and max(len(b) for _, b in nodes) <= (m + 1) // 2
        assert want["trees"][0].feat[0] == 1 and want["trees"][0].cat[0] == best[2]   # the root of the first tree is that candidate
    booster.close()


@pytest.mark.parametrize("threshold", [1, 2])
def test_max_cat_threshold_binds(ctx, threshold):
    """ten eligible categories ((m + 1) / 2 = 5), three of them with the high labels: the sets stop at max_cat_threshold members"""
    X, y, off = two_columns(41, list(range(10)), [60] * 10, [3 if i in TC.MEMBERS else 0 for i in range(10)])
    booster, hist, want = both(ctx, X, y, off, dict(SMALL, max_cat_threshold=threshold))
    sizes = [len(b) for _, b in cat_nodes(want, 1)]
    assert sizes and max(sizes) == threshold
    booster.close()


def test_a_winner_from_direction_1(ctx):
    """ten categories, two of them (3 and 8) with the LOW labels: they have the highest keys (a low label's gradient is positive), and
    the set {3, 8} is reachable only as the last two bins of the order - its complement has eight members, max_num is five"""
    X, y, off = two_columns(43, list(range(10)), [60] * 10, [0 if i in (3, 8) else 3 for i in range(10)])
    best, keys = root_search(X, y, off, 1, SMALL)
    assert best[3] == 256 + 1 and best[2] == [3, 8] and sorted(b for _, b in keys[-2:]) == [3, 8]
    booster, hist, want = both(ctx, X, y, off, SMALL)
    t = want["trees"][0]
    assert t.feat[0] == 1 and t.cat[0] == [3, 8]
    words = [ln for ln in hist["model"].decode().split("\n") if ln.startswith("cat_threshold=")][0].split("=")[1].split()
    assert int(words[0]) == (1 << 3) | (1 << 8)
    booster.close()


def test_254_bins_of_300_categories_and_bin_255_goes_right(ctx):
    """ids 0 ... 253 hold 11 cells each, ids 254 ... 299 one cell each (no bin), 60 cells are NaN; the validation set holds the rare ids,
    NaN, a negative id and an id never seen: bin 255 goes right in the training rows and in the validation walk"""
    ids = list(range(300))
    base = [3 if i % 3 == 0 else 0 for i in ids]
    X, y, off = two_columns(51, ids, [11] * 254 + [1] * 46, base, nan=60)
    VX, vy, voff = two_columns(52, ids, [2] * 300, base, nan=30)
    VX[:4, 1] = [-5.0, 4000.0, 32764.0, -0.5]
    cfg = dict(SMALL, cat_smooth=2.0, min_data_per_group=20, early_stopping=2)
    booster, hist, want = both(ctx, X, y, off, cfg, valid=(VX, vy, voff))
    assert list(want["kept"][1]) == list(range(254)) and want["nbins"][1] == 254
    assert (TC.bin_cat_column(X[:, 1], want["kept"][1]) == 255).sum() == 46 + 60
    assert (TC.bin_cat_column(VX[:, 1], want["kept"][1]) == 255).sum() >= 46 * 2 + 30
    nodes = cat_nodes(want, 1)
    assert nodes and max(len(b) for _, b in nodes) > 4
    booster.close()


def test_twin_categories_order_by_the_lower_bin(ctx):
    """categories 2 and 5 each own eight whole groups with the same label sequences: at the first iteration every score is 0, so their
    (G, H, count) are the same bits and their keys tie.  Categories 1 (high labels) and 7 (low labels) share the mixed groups, 60 rows
    each: below min_data_per_group = 100 alone, admitted together with ONE twin - the first in the order behind category 1 (direction
    0) or the last before category 7 (direction 1).  Which twin that is falls to the bin: the lower one comes first"""
    rng = np.random.default_rng(61)
    seqs = [rng.integers(0, 5, 10).astype(np.float64) for _ in range(8)]
    cat, y, sizes = [], [], []
    for twin in (5.0, 2.0):
        for s in seqs:
            cat += [twin] * 10
            y += list(s)
            sizes.append(10)
    for _ in range(12):
        c = rng.permutation(np.repeat([1.0, 7.0], 5))
        cat += list(c)
        y += list(np.where(c == 1.0, rng.integers(3, 5, 10), rng.integers(0, 2, 10)).astype(np.float64))
        sizes.append(10)
    # four more categories without rows enough to be eligible: K = 8 > max_cat_to_onehot
    for extra in (10.0, 11.0, 12.0, 13.0):
        cat += [extra] * 5
        y += [0.0, 1.0, 2.0, 3.0, 4.0]
        sizes.append(5)
    cat, y = np.array(cat), np.array(y)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = np.column_stack([rng.normal(size=len(y)), cat])
    cfg = dict(SMALL, cat_smooth=10.0, min_data_per_group=100, iterations=1)
    best, keys = root_search(X, y, off, 1, cfg)
    kept = list(TC.kept_categories(cat))
    b2, b5 = kept.index(2), kept.index(5)
    by_bin = {b: k for k, b in keys}
    assert len(keys) == 4 and T.bits(by_bin[b2]) == T.bits(by_bin[b5])                # the keys really tie
    order = [b for _, b in keys]
    assert order.index(b2) + 1 == order.index(b5)                                     # the lower bin first
    assert best is not None and len(best[2]) == 2 and len(set(best[2]) & {b2, b5}) == 1
    assert (b2 if best[3] < 256 else b5) in best[2]
    booster, hist, want = both(ctx, X, y, off, cfg)
    t = want["trees"][0]
    assert t.feat[0] == 1 and t.cat[0] == best[2]
    booster.close()


def test_bitset_words(ctx):
    """kept ids on both sides of the word boundaries and the largest id there is; the high labels sit on 31, 64 and 32764"""
    ids = [0, 31, 32, 63, 64, 100, 32764]
    X, y, off = two_columns(71, ids, [70] * 7, [3 if i in (31, 64, 32764) else 0 for i in ids])
    booster, hist, want = both(ctx, X, y, off, SMALL)
    assert list(want["kept"][1]) == ids
    assert want["trees"][0].feat[0] == 1 and want["trees"][0].cat[0] == [1, 4, 6]
    block = hist["model"].decode().split("Tree=0\n")[1].split("\n\n")[0]
    lines = dict(ln.split("=", 1) for ln in block.split("\n"))
    bounds, words = [int(v) for v in lines["cat_boundaries"].split()], [int(v) for v in lines["cat_threshold"].split()]
    assert bounds[:2] == [0, 1024] and len(words) == bounds[-1]
    assert words[0] == 1 << 31 and words[1] == 0 and words[2] == 1 and words[1023] == 1 << (32764 % 32) and not any(words[3:1023])
    P = np.zeros((len(ids) + 3, 2))
    P[:, 1] = ids + [30.0, 65.0, 32763.0]
    got = booster.predict(P)
    assert np.array_equal(T.bits(got), T.bits(OracleForest.from_lightgbm_text(hist["model"]).predict(P)))
    assert got[1] != got[7] and got[4] != got[8] and got[6] != got[9]   # a member (left at the root) and its neighbour without a bin
    booster.close()


# ------------------------------------------------------------------ a mixed forest
MIXED = {"iterations": 6, "sampling": 0.8, "maxDepth": 3, "numLeaves": 16, "early_stopping": 3, "categorical": [8, 9]}


def mixed_valid():
    VX, vy, voff = TC.dataset(107, rows=300, rare=False)
    return TC.odd_cells(VX, 8)[0], vy, voff


@pytest.mark.parametrize("rows", [2047, 2048, 2049])
def test_mixed_forest_on_both_sides_of_the_tiles(ctx, rows):
    """train_reference.dataset's 8 columns plus 2 categorical ones, labels that follow the id SET {1, 4, 7}; depth and leaf limits,
    column subsets, a validation set with cells that have no bin, early stopping"""
    X, y, off = TC.dataset(7, rows=rows)
    booster, hist, want = both(ctx, X, y, off, MIXED, valid=mixed_valid())
    trees = want["trees"]
    assert any(t.cat for t in trees) and any(t.dt[n] != 9 for t in trees for n in range(len(t.dt)))
    assert any(sorted(b) == list(TC.MEMBERS) for c, b in cat_nodes(want, 8))
    assert all(max(t.depth.values()) <= 3 for t in trees) and any(t.num_leaves == 8 for t in trees)
    booster.close()


def test_it_is_worth_having(ctx):
    """The labels follow the id set {1, 4, 7} of column 8.  Held-out ndcg@10 (1 000 rows of TC.dataset(8), mrk_model_eval) of the fit
    with columns 8 and 9 categorical against the same fit with them numeric.  The restatement's two models on the CPU (the oracle's
    reader, eval_reference): categorical 0.97417806, numeric 0.71352382.  The condition is the order, and device == restatement."""
    X, y, off = TC.dataset(7, rows=2048)
    HX, hy, hoff = TC.dataset(8, rows=1000, rare=False)
    values = {}
    for name, cats in (("categorical", [8, 9]), ("numeric", [])):
        cfg = dict(MIXED, categorical=cats)
        booster, hist, want = both(ctx, X, y, off, cfg, valid=mixed_valid())
        values[name] = evaluate(booster, HX, hy, hoff, metrics=(("ndcg", 10),), seed=0)[0]["value"]
        ref = E.mean(E.per_group(E.NDCG, 10, OracleForest.from_lightgbm_text(want["model"]).predict(HX), hy, hoff))
        print(name, values[name], ref)
        assert T.bits(values[name]) == T.bits(ref)
        booster.close()
    assert values["categorical"] > values["numeric"]


# ------------------------------------------------------------------ refusals, the old path, upload pieces
def test_refusals(ctx):
    X, y, off = two_columns(81, [0, 1, 2], [50] * 3, [3, 0, 1])
    with pytest.raises(_native.MrkError) as e:
        fit_lambdamart(X, y, off, ctx=ctx, categorical=[1, 2])
    assert e.value.status == _native.ERR_INVALID_ARG and "index 2" in e.value.message
    B = X.copy()
    B[7, 1] = 32765.0
    with pytest.raises(_native.MrkError) as e:
        fit_lambdamart(B, y, off, ctx=ctx, categorical=[1])
    assert e.value.status == _native.ERR_UNSUPPORTED and "32765" in e.value.message and "row 7" in e.value.message
    with pytest.raises(_native.MrkError) as e:
        fit_lambdamart(X, y, off, valid=(B, y, off), ctx=ctx, categorical=[1])
    assert e.value.status == _native.ERR_UNSUPPORTED and "32765" in e.value.message
    booster, hist = fit_lambdamart(B, y, off, ctx=ctx, iterations=1, min_data_in_leaf=5)   # numeric: any finite cell is a value
    assert hist["iterations_run"] == 1
    booster.close()


def test_without_a_categorical_column_the_bytes_are_train_references(ctx):
    X, y, off = T.dataset(1, rows=700)
    cfg = {"iterations": 3, "min_data_in_leaf": 5}
    want = T.fit(X, y, off, cfg=cfg)
    for extra in ({}, {"categorical": categorical_columns([("a", 0, 1, "single"), ("v", 1, 7, "vector")])}, {"categorical": None, "cat_l2": 3.0, "cat_smooth": 2.0}):
        booster, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg, **extra)
        assert hist["model"] == want["model"], first_difference(hist["model"], want["model"])
        assert np.array_equal(T.bits(hist["scores"]), T.bits(want["scores"]))
        booster.close()


def test_upload_pieces(ctx, monkeypatch):
    X, y, off = TC.dataset(5, rows=900)
    valid = mixed_valid()
    cfg = dict(MIXED, iterations=2, min_data_per_group=20)
    models = []
    for piece in (None, "37"):
        if piece:
            monkeypatch.setenv("MRK_TRAIN_PIECE_ROWS", piece)
        booster, hist = fit_lambdamart(X, y, off, valid=valid, ctx=ctx, **cfg)
        models.append((hist["model"], T.bits(hist["scores"]).tobytes(), T.bits(hist["valid_scores"]).tobytes()))
        booster.close()
    assert models[0] == models[1] and b"cat_threshold=" in models[0][0]
    want = TC.fit(X, y, off, valid=valid, cfg=cfg)
    assert models[0][0] == want["model"]
