"""Categorical splits of the xgboost backend (include/mrk.h steps 2cx, 5cx and the model text) restated in Python / numpy
on top of the unchanged train_xgb_reference: a "c" column's cells become categories as the model's f32 test sees them, the kept ones
get bins 0 ... K - 1, every other one bin 254 ("other", always left), NaN bin 255; a candidate is a set R of kept bins that goes RIGHT.
Every sum over rows is an int64 sum; every comparison of gains is of f64 values computed in the header's order."""
import os
import re

import numpy as np

import eval_reference as E
import train_bias_reference as B
import train_reference as T
import train_xgb_reference as TX

NAN_BIN, OTHER_BIN, MAX_CATEGORY = 255, 254, 32764
MAX_CAT_TO_ONEHOT, MAX_CAT_THRESHOLD = 4, 64
_hpp = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metarank_amd", "csrc", "train.hpp")).read()
LDS_MASKS = int(re.search(r"TRAIN_LEVEL_LDS_MASKS = (\d+);", _hpp).group(1))       # masks of a level the routing kernel holds in LDS


# ------------------------------------------------------------------ 2cx. bins of a "c" column
def category(column):
    """per cell: its category, -1 for NaN, -2 for a cell the model sends left whatever the set is"""
    x = np.asarray(column, dtype=np.float64)
    if np.isinf(x).any():
        raise ValueError("an infinite cell")
    with np.errstate(over="ignore"):
        v = x.astype(np.float32)
    out = np.full(len(v), -2, dtype=np.int64)
    out[np.isnan(v)] = -1
    ok = (v >= np.float32(0.0)) & (v < np.float32(2.0 ** 24))
    ids = v[ok].astype(np.int64)                               # truncates
    out[ok] = np.where(ids > MAX_CATEGORY, -2, ids)
    return out


def kept_categories(column, max_bin=255):
    c = category(column)
    ids, counts = np.unique(c[c >= 0], return_counts=True)
    order = sorted(range(len(ids)), key=lambda k: (-int(counts[k]), int(ids[k])))[:max(max_bin - 2, 0)]
    return np.sort(ids[order]).astype(np.int64)


def bin_column(column, kept):
    c = category(column)
    b = np.full(len(c), OTHER_BIN, dtype=np.uint8)
    for k, cat in enumerate(kept):
        b[c == cat] = k
    b[c == -1] = NAN_BIN
    return b


# ------------------------------------------------------------------ 5cx. the candidates of a "c" column
def right_sets(G, H, C, K, e_g, e_h, lam):
    """the sets R in the order a tie is decided: direction 0 by ascending size, then direction 1"""
    if K < MAX_CAT_TO_ONEHOT:
        return [(b,) for b in range(K)]
    den = {b: float(T.real(H[b], e_h)) + lam for b in range(K)}
    order = sorted((b for b in range(K) if C[b] > 0 and den[b] > 0.0), key=lambda b: (float(T.real(G[b], e_g)) / den[b], b))
    n = min(MAX_CAT_THRESHOLD, len(order))
    return [tuple(order[:i]) for i in range(1, n + 1)] + [tuple(order[len(order) - i:]) for i in range(1, n + 1)]


def best_cat_split(G, H, C, K, col, e_g, e_h, cfg):
    """-> (gain, col, R, nan_left, left sums) or None; G, H, C: the 256 bins of one (node, column)"""
    lam, gamma, mcw = float(cfg["lambda"]), float(cfg["gamma"]), float(cfg["min_child_weight"])
    tg, th, tc = int(G.sum()), int(H.sum()), int(C.sum())
    ng, nh, nc = int(G[NAN_BIN]), int(H[NAN_BIN]), int(C[NAN_BIN])
    f = lambda q, e: np.float64(T.real(q, e))
    term = lambda qg, qh: (f(qg, e_g) * f(qg, e_g)) / (f(qh, e_h) + lam)
    best = None
    with np.errstate(divide="ignore", invalid="ignore"):
        parent = term(tg, th)
        for R in right_sets(G, H, C, K, e_g, e_h, lam):
            sg, sh, sc = (sum(int(a[b]) for b in R) for a in (G, H, C))
            for nan_left in ((0, 1) if nc > 0 else (0,)):      # NaN right first: it wins a tie
                rg, rh, rc = (sg, sh, sc) if nan_left else (sg + ng, sh + nh, sc + nc)
                lg, lh, lc = tg - rg, th - rh, tc - rc         # "other" (bin 254) is on the left of every candidate
                gain = (term(lg, lh) + term(rg, rh)) - parent
                if lc >= 1 and rc >= 1 and f(lh, e_h) >= mcw and f(rh, e_h) >= mcw and gain > gamma and (best is None or gain > best[0]):
                    best = (float(gain), col, R, nan_left, (lg, lh, lc))
    return best


def best_split(hist, nbins, is_cat, e_g, e_h, cfg):
    """across columns: the highest gain, then the lowest column"""
    best = TX._best_split(hist, [0 if c else n for n, c in zip(nbins, is_cat)], e_g, e_h, cfg)      # the "q" columns: step 5x
    for col in np.flatnonzero(is_cat):
        c = best_cat_split(hist[0][col], hist[1][col], hist[2][col], nbins[col], int(col), e_g, e_h, cfg)
        if c is not None and (best is None or c[0] > best[0] or (c[0] == best[0] and c[1] < best[1])):
            best = c
    return best


def goes_left(t, node, cb):
    """a column's bins -> which of them leave `node` to the left"""
    if node in t.cats:
        return np.where(cb == NAN_BIN, bool(t.default_left[node]), ~np.isin(cb, t.cats[node]))
    return (cb <= t.bin[node]) | ((cb == NAN_BIN) & bool(t.default_left[node]))


def grow_tree(binsT, nbins, is_cat, bounds, qg, qh, e_g, e_h, sample, cfg):
    """TX.grow_tree with best_split; t.cats: node -> the bins of its right set"""
    rows, cols = len(qg), len(nbins)
    node_of = np.zeros(rows, dtype=np.int64)
    t = TX.Tree()
    t.cats = {}
    t.add(TX.ROOT_PARENT, 0)
    totals = {0: (int(qg[sample].sum()), int(qh[sample].sum()), int(sample.sum()))}
    level, d = [0], 0
    while level:
        nxt = []
        for node in level:
            if d >= int(cfg["maxDepth"]) or totals[node][2] < 2:
                continue
            idx = np.flatnonzero((node_of == node) & sample)
            best = best_split(T._histogram(binsT, list(range(cols)), idx, qg, qh), nbins, is_cat, e_g, e_h, cfg)
            if best is None:
                continue
            gain, col, b, nan_left, (QGL, QHL, CL) = best
            t.col[node], t.default_left[node], t.loss_change[node] = col, nan_left, np.float32(gain)
            if is_cat[col]:
                t.cats[node] = b                               # (cond stays 0)
            else:
                t.bin[node], t.cond[node] = b, np.float32(bounds[col][b])
            l, r = t.add(node, d + 1), t.add(node, d + 1)
            t.left[node], t.right[node] = l, r
            mine, left = node_of == node, goes_left(t, node, binsT[col])
            node_of[mine & left], node_of[mine & ~left] = l, r
            tg, th, tc = totals[node]
            totals[l], totals[r] = (QGL, QHL, CL), (tg - QGL, th - QHL, tc - CL)
            nxt += [l, r]
        level, d = nxt, d + 1
    if t.num_nodes == 1:
        return None, None
    for node in range(t.num_nodes):
        t.weigh(node, totals[node][0], totals[node][1], e_g, e_h, float(cfg["lambda"]), float(cfg["learningRate"]))
    return t, node_of


def route(t, binsT, rows):
    node_of = np.zeros(rows, dtype=np.int64)
    for node in range(t.num_nodes):                            # a parent comes before its children
        if t.left[node] >= 0:
            mine, left = node_of == node, goes_left(t, node, binsT[t.col[node]])
            node_of[mine & left], node_of[mine & ~left] = t.left[node], t.right[node]
    return node_of


# ------------------------------------------------------------------ the model text
def write_model(trees, cols, feature_types, kept):
    """TX.write_model's bytes with the categorical arrays, split_type and feature_types filled in"""
    empty = '"categories":[],"categories_nodes":[],"categories_segments":[],"categories_sizes":[],'
    parts = TX.write_model(trees, cols).decode().split(empty)
    lst = lambda a: ",".join(str(int(x)) for x in a)
    for i, t in enumerate(trees):
        nodes = sorted(t.cats)
        ids = [[int(kept[t.col[n]][b]) for b in sorted(t.cats[n])] for n in nodes]
        seg = np.concatenate([[0], np.cumsum([len(a) for a in ids])]).astype(int)
        parts[i] += '"categories":[%s],"categories_nodes":[%s],"categories_segments":[%s],"categories_sizes":[%s],' % (
            lst(sum(ids, [])), lst(nodes), lst(seg[:-1]), lst(len(a) for a in ids))
        zeros = '"split_type":[%s]' % lst([0] * t.num_nodes)
        assert parts[i + 1].count(zeros) >= 1
        parts[i + 1] = parts[i + 1].replace(zeros, '"split_type":[%s]' % lst(int(n in t.cats) for n in range(t.num_nodes)), 1)
    text = "".join(parts)
    if "c" in feature_types:
        text = text.replace('"feature_types":[]', '"feature_types":[%s]' % ",".join('"%s"' % f for f in feature_types), 1)
    return text.encode("utf-8")


# ------------------------------------------------------------------ the fit
def _fit(X, labels, offsets, valid, cfg, feature_types):
    """TX.fit's loop over the bins, trees and model text above"""
    cfg = TX.parse_config(cfg)
    X = np.asarray(X, dtype=np.float64)
    rows, cols = X.shape
    y, offsets = np.asarray(labels, dtype=np.int64), [int(o) for o in offsets]
    is_cat = np.array([f == "c" for f in feature_types], dtype=bool)
    mb = int(cfg["max_bin"])
    kept = [kept_categories(X[:, c], mb) if is_cat[c] else None for c in range(cols)]
    bounds = [None if is_cat[c] else TX.bin_bounds(X[:, c], mb) for c in range(cols)]
    nbins = [len(kept[c]) if is_cat[c] else len(bounds[c]) + 1 for c in range(cols)]
    bins_of = lambda M: [bin_column(M[:, c], kept[c]) if is_cat[c] else TX.bin_column(M[:, c], bounds[c]) for c in range(cols)]
    binsT = bins_of(X)
    scores = np.full(rows, 0.5, dtype=np.float32)
    if valid is not None:
        VX, vy, voff = np.asarray(valid[0], dtype=np.float64), np.asarray(valid[1], dtype=np.float64), [int(o) for o in valid[2]]
        vbinsT, vscores = bins_of(VX), np.full(len(vy), 0.5, dtype=np.float32)
    trees, history = [], []
    best_it, best_metric, best_scores, best_vscores = 0, None, scores.copy(), None if valid is None else vscores.copy()
    for it in range(int(cfg["iterations"])):
        g, h = T.gradients(scores.astype(np.float64), y, offsets, float(cfg["sigma"]), int(cfg["truncation"]))
        gmax, hmax = float(np.max(np.abs(g))), float(np.max(h))
        if gmax == 0.0:
            break
        e_g, e_h = T.exponent(gmax, rows), T.exponent(hmax, rows)
        sample = TX.row_sample(rows, float(cfg["sampling"]), int(cfg["seed"]), it)
        t, node_of = grow_tree(binsT, nbins, is_cat, bounds, T.quantise(g, e_g), T.quantise(h, e_h), e_g, e_h, sample, cfg)
        if t is None:
            break
        trees.append(t)
        lv = np.array(t.cond, dtype=np.float32)
        scores = scores + lv[node_of]
        if valid is None:
            best_it, best_scores = len(trees), scores.copy()
            continue
        vscores = vscores + lv[route(t, vbinsT, len(vy))]
        m = E.mean(E.per_group(E.NDCG, int(cfg["ndcgCutoff"]), vscores.astype(np.float64), vy, voff, relpow=True, nolabels=1.0))
        history.append(m)
        if best_metric is None or m > best_metric:
            best_it, best_metric, best_scores, best_vscores = len(trees), m, scores.copy(), vscores.copy()
        elif len(trees) - best_it >= int(cfg["early_stopping"]):
            break
    return {"model": write_model(trees[:best_it], cols, feature_types, kept), "iterations_run": len(trees), "best_iteration": best_it,
            "history": np.array(history, dtype=np.float64), "scores": best_scores.astype(np.float64),
            "valid_scores": None if valid is None else best_vscores.astype(np.float64), "trees": trees, "kept": kept, "bins": binsT, "bins_of": bins_of}


def fit(X, labels, offsets, valid=None, cfg=None):
    """cfg as the device's, feature_types and position_bias included (step 3b: train_bias_reference, whose loop finds this one as TX.fit)"""
    cfg = dict(cfg or {})
    ft = cfg.pop("feature_types", None) or ["q"] * np.asarray(X).shape[1]
    if "position_bias" not in cfg:
        return _fit(X, labels, offsets, valid, cfg, ft)
    plain, TX.fit = TX.fit, lambda X, labels, offsets, valid=None, cfg=None: _fit(X, labels, offsets, valid, cfg, ft)
    try:
        return B.fit(X, labels, offsets, valid=valid, cfg=cfg)
    finally:
        TX.fit = plain


# ------------------------------------------------------------------ data and cases of the tests
SPECIAL_CELLS = (np.nan, -1.0, 2.9999999999, 40000.0, 2.0 ** 24)      # NaN; "other"; category 2; beyond every bitset; no valid category
CAT_COLUMNS = (3, 5, 7, 0)                                             # the columns of T.dataset that become "c" columns, in this order
# name -> (what the case is there for, distinct ids per "c" column, NaN share, rows, valid rows, config)
CASES = {
    "k3": ("onehot", (3,), 0.0, 2000, 0, {"iterations": 4, "maxDepth": 4, "sampling": 0.8}),
    "k6": ("partition", (6,), 0.0, 2000, 0, {"iterations": 4, "maxDepth": 4, "sampling": 1.0}),
    "k70": ("word2", (70,), 0.0, 2000, 0, {"iterations": 4, "maxDepth": 5, "sampling": 0.8}),
    "nan": ("default_left", (6, 3), 0.15, 2000, 0, {"iterations": 4, "maxDepth": 4, "sampling": 1.0}),
    "deep": ("overflow", (300, 300, 70, 70), 0.0, 3000, 0, {"iterations": 2, "maxDepth": 9, "sampling": 1.0, "min_child_weight": 1e-6, "lambda": 0.01}),
    "valid": ("partition", (300, 6), 0.02, 2000, 600, {"iterations": 8, "maxDepth": 4, "sampling": 0.8, "early_stopping": 8}),
    "bias": ("partition", (70, 3), 0.0, 2000, 0, {"iterations": 3, "maxDepth": 4, "sampling": 0.8, "position_bias": {}}),
}


def case_data(name, seed=0, rows=None):
    """-> (X, y, offsets, feature_types): T.dataset with "c" columns whose categories move the label; every "c" column holds SPECIAL_CELLS"""
    _, n_ids, nan_share, case_rows, _, _ = CASES[name]
    rows = rows or case_rows
    X, y, off = T.dataset(11 + seed, rows=rows)
    rng = np.random.default_rng([len(name), seed, rows])
    ft = ["q"] * X.shape[1]
    for col, n in zip(CAT_COLUMNS, n_ids):
        n -= n == 3                                                                       # (2.9999999999 is category 3 as an f32: K = 3 with ids 0, 1)
        ids = (n * rng.random(rows) ** (2.0 if n > 100 else 1.0)).astype(np.int64)       # many ids: the low ones are frequent
        y = y + (rng.normal(size=n) * 1.5)[ids]
        X[:, col] = ids * (3 if n > 100 else 1) + 0.25                                    # (the category truncates; 300 ids reach 897)
        X[rng.choice(rows, 2 * len(SPECIAL_CELLS), replace=False), col] = SPECIAL_CELLS * 2
        gone = rng.random(rows) < nan_share
        X[gone, col], y = np.nan, y + 1.5 * gone
        ft[col] = "c"
    return X, np.clip(np.floor(y), 0, 4), off, ft


def case_valid(name):
    """the validation set of a case: another seed, and ids the training set never saw"""
    if not CASES[name][4]:
        return None
    VX, vy, voff, _ = case_data(name, seed=1, rows=CASES[name][4])
    VX[::7, CAT_COLUMNS[0]] += 1000.0
    return VX, vy, voff


def case_config(name):
    return dict(CASES[name][5], backend="xgboost", feature_types=case_data(name)[3])


def case_fit(name):
    X, y, off, _ = case_data(name)
    return fit(X, y, off, valid=case_valid(name), cfg=case_config(name))


def predict(r, X):
    """the kept trees over the restatement's own bins and routing: f32 sums from the base_score, widened"""
    binsT, s = r["bins_of"](np.asarray(X, dtype=np.float64)), np.full(len(X), 0.5, dtype=np.float32)
    for t in r["trees"][:r["best_iteration"]]:
        s = s + np.array(t.cond, dtype=np.float32)[route(t, binsT, len(X))]
    return s.astype(np.float64)


def purposes(r):
    """what a fit shows, from the restatement's trees alone: the set of CASES' first entries it produces"""
    out = set()
    for t in r["trees"]:
        level = {}
        for n, R in t.cats.items():
            K = len(r["kept"][t.col[n]])
            out |= {"onehot"} if K < MAX_CAT_TO_ONEHOT else {"partition"} if len(R) > 1 else set()
            out |= ({"word2"} if max(R) >= 64 else set()) | ({"default_left"} if t.default_left[n] else set())
            level[t.depth[n]] = level.get(t.depth[n], 0) + 1
        out |= {"overflow"} if max(level.values(), default=0) > LDS_MASKS else set()
    return out
