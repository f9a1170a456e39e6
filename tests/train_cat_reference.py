"""Categorical columns of the LambdaMART fit (include/mrk.h steps 2c and 5c) restated in Python / numpy beside
tests/train_reference.py, which stays as it is: gradients, quantisation, exponents, feature subsets, the numeric bins, the tree
numbering, the leaf outputs and the numeric split search are imported from there; the categorical bins, the categorical split
search, the tree growth / routing with bin masks, the model text with its cat_* lines and the fit are restated here.  With
`categorical == []` fit() returns train_reference.fit's bytes.  Every sum over rows is an int64 sum, every real operation one
correctly rounded f64 operation: numpy's evaluation order cannot change a bit."""
import numpy as np

import eval_reference as E
import train_reference as T

MAX_CATEGORY = 32764          # 0x7FFC: the largest id the scorers' categorical cell holds exactly
NAN_BIN = T.NAN_BIN

DEFAULTS = dict(T.DEFAULTS, categorical=[], max_cat_to_onehot=4, max_cat_threshold=32, cat_smooth=10.0, cat_l2=10.0, min_data_per_group=100)


def parse_config(cfg=None):
    out = dict(DEFAULTS)
    for k, v in (cfg or {}).items():
        if k not in DEFAULTS:
            raise KeyError(k)
        if v is not None:
            out[k] = v
    cats = [int(c) for c in out["categorical"]]
    if len(set(cats)) != len(cats) or any(c < 0 for c in cats):
        raise ValueError("categorical")
    out["categorical"] = cats
    return out


# ------------------------------------------------------------------ 2c. bins of a categorical column
def categories(column):
    """the category of every cell (int64), -1 where it has none: NaN, and trunc(x) < 0"""
    x = np.asarray(column, dtype=np.float64)
    if np.isinf(x).any():
        raise ValueError("infinite cell")
    c = np.where(np.isnan(x), -1.0, np.trunc(np.where(np.isnan(x), 0.0, x)))
    if (c > MAX_CATEGORY).any():
        raise OverflowError("a category beyond %d" % MAX_CATEGORY)
    return np.where(c < 0, -1, c).astype(np.int64)


def kept_categories(column, max_bin=255):
    """the ids that get a bin of their own, ascending: the min(distinct, max_bin - 1) most frequent, ties to the lower id"""
    c = categories(column)
    ids, counts = np.unique(c[c >= 0], return_counts=True)
    order = sorted(range(len(ids)), key=lambda i: (-int(counts[i]), int(ids[i])))[:max_bin - 1]
    return np.array(sorted(int(ids[i]) for i in order), dtype=np.int64)


def bin_cat_column(column, kept):
    """bin = the position of the cell's category among the kept ids; 255 for everything else"""
    c = categories(column)
    out = np.full(len(c), NAN_BIN, dtype=np.uint8)
    if len(kept):
        pos = np.searchsorted(kept, c)
        hit = (pos < len(kept)) & (kept[np.minimum(pos, len(kept) - 1)] == c)
        out[hit] = pos[hit]
    return out


def cat_feature_info(kept):
    return ":".join(str(int(i)) for i in kept) if len(kept) else "none"


# ------------------------------------------------------------------ 5c. the split search on a categorical column
def _gain(QGL, QHL, tg, th, e_g, e_h, l2_sides, l2_parent):
    GL, HL = float(T.real(QGL, e_g)), float(T.real(QHL, e_h))
    GR, HR = float(T.real(tg - QGL, e_g)), float(T.real(th - QHL, e_h))
    Gt, Ht = float(T.real(tg, e_g)), float(T.real(th, e_h))
    with np.errstate(divide="ignore", invalid="ignore"):
        gain = float((np.float64(GL * GL) / np.float64(HL + l2_sides) + np.float64(GR * GR) / np.float64(HR + l2_sides)) - np.float64(Gt * Gt) / np.float64(Ht + l2_parent))
    return gain, HL, HR


def cat_keys(G, H, C, K, e_g, e_h, cfg):
    """[(key, bin)] of the eligible bins, ascending"""
    cs = float(cfg["cat_smooth"])
    out = []
    for b in range(K):
        if float(int(C[b])) >= cs:
            out.append((float(T.real(int(G[b]), e_g)) / (float(T.real(int(H[b]), e_h)) + cs), b))
    return sorted(out)


def best_cat_split(G, H, C, K, col, e_g, e_h, cfg):
    """(gain, col, sorted left bins, code, (QGL, QHL, CL)) of the best admitted candidate of one column's histogram or None.
    code: the bin (one-vs-rest) or direction * 256 + (i - 1) (sorted); the lowest code wins among equal gains"""
    l2, mdl, msh = float(cfg["lambda_l2"]), int(cfg["min_data_in_leaf"]), float(cfg["min_sum_hessian"])
    tg, th, tc = int(G.sum()), int(H.sum()), int(C.sum())
    cands = []                                             # (code, bins) in ascending code
    if K <= int(cfg["max_cat_to_onehot"]):
        l2_sides, min_cnt = l2, mdl
        cands = [(b, [b]) for b in range(K)]
    else:
        l2_sides, min_cnt = l2 + float(cfg["cat_l2"]), max(mdl, int(cfg["min_data_per_group"]))
        order = [b for _, b in cat_keys(G, H, C, K, e_g, e_h, cfg)]
        m = len(order)
        max_num = min(int(cfg["max_cat_threshold"]), (m + 1) // 2)
        cands = [(i - 1, order[:i]) for i in range(1, max_num + 1)] + [(256 + i - 1, order[m - i:]) for i in range(1, max_num + 1)]
    best = None
    for code, bins in cands:
        QGL, QHL, CL = int(G[bins].sum()), int(H[bins].sum()), int(C[bins].sum())
        gain, HL, HR = _gain(QGL, QHL, tg, th, e_g, e_h, l2_sides, l2)
        if CL >= min_cnt and tc - CL >= min_cnt and HL >= msh and HR >= msh and gain > 0.0 and (best is None or gain > best[0]):
            best = (gain, col, sorted(bins), code, (QGL, QHL, CL))
    return best


def _best_split(hist, subset, nbins, is_cat, e_g, e_h, cfg):
    """the best candidate over the subset's columns: the highest gain, then the lowest column.  A numeric candidate is
    train_reference's tuple (gain, col, b, nan_left, sums); a categorical one carries the list of left bins in place of b and
    nan_left = None"""
    G, H, C = hist
    best = None
    for j, col in enumerate(subset):
        if is_cat[col]:
            c = best_cat_split(G[j], H[j], C[j], int(nbins[col]), col, e_g, e_h, cfg)
            c = None if c is None else (c[0], c[1], c[2], None, c[4])
        else:
            c = T._best_split((G[j:j + 1], H[j:j + 1], C[j:j + 1]), [col], nbins, e_g, e_h, cfg)
        if c is not None and (best is None or c[0] > best[0]):
            best = c
    return best


# ------------------------------------------------------------------ one tree
def goes_left(t, n, b):
    """bins b (array) at node n"""
    if n in t.cat:
        return np.isin(b, t.cat[n]) & (b != NAN_BIN)
    return (b <= t.bin[n]) | ((b == NAN_BIN) & ((t.dt[n] & 2) != 0))


def grow_tree(binsT, nbins, is_cat, bounds, qg, qh, e_g, e_h, subset, cfg):
    """train_reference.grow_tree with categorical nodes: t.cat[node] = the sorted bins that go left"""
    rows = len(qg)
    l2, lr = float(cfg["lambda_l2"]), float(cfg["learningRate"])
    leaf_of = np.zeros(rows, dtype=np.int64)
    t = T.Tree()
    t.cat = {}
    search = lambda idx: _best_split(T._histogram(binsT, subset, idx, qg, qh), subset, nbins, is_cat, e_g, e_h, cfg)
    totals = {0: (int(qg.sum()), int(qh.sum()), rows)}
    cand = {0: search(np.arange(rows))}
    while t.num_leaves < int(cfg["numLeaves"]):
        leaf, best = None, None
        for lf in sorted(cand):
            c = cand[lf]
            if c is not None and t.depth[lf] < int(cfg["maxDepth"]) and (best is None or c[0] > best[0]):
                leaf, best = lf, c
        if best is None:
            break
        gain, col, b, nan_left, (QGL, QHL, CL) = best
        tg, th, tc = totals[leaf]
        v, w = T.leaf_output(tg, th, e_g, e_h, l2, lr)
        t.ivalue.append(v), t.iweight.append(w), t.icount.append(tc)
        node = len(t.feat)
        if nan_left is None:
            new = t.split(leaf, col, 0, float(len(t.cat)), 0, gain)      # threshold: the ordinal among the tree's categorical nodes
            t.dt[node] = 9                                               # categorical, missing type NaN
            t.cat[node] = list(b)
        else:
            new = t.split(leaf, col, b, float(bounds[col][b]), nan_left, gain)
        left = goes_left(t, node, binsT[col])
        leaf_of[(leaf_of == leaf) & ~left] = new
        totals[leaf], totals[new] = (QGL, QHL, CL), (tg - QGL, th - QHL, tc - CL)
        for lf in (leaf, new):
            idx = np.flatnonzero(leaf_of == lf)
            assert len(idx) == totals[lf][2]
            cand[lf] = search(idx) if t.depth[lf] < int(cfg["maxDepth"]) else None
    if t.num_leaves == 1:
        return None, None
    for lf in range(t.num_leaves):
        t.value[lf], t.weight[lf] = T.leaf_output(totals[lf][0], totals[lf][1], e_g, e_h, l2, lr)
        t.count[lf] = totals[lf][2]
    return t, leaf_of


def route(t, binsT, rows):
    out = np.empty(rows, dtype=np.int64)
    for i in range(rows):
        n = 0
        while n >= 0:
            b = int(binsT[t.feat[n]][i])
            if n in t.cat:
                left = b != NAN_BIN and b in t.cat[n]
            else:
                left = (b <= t.bin[n]) or (b == NAN_BIN and (t.dt[n] & 2) != 0)
            n = t.left[n] if left else t.right[n]
        out[i] = ~n
    return out


# ------------------------------------------------------------------ the model text
def cat_lines(t, kept):
    """(num_cat, cat_boundaries, cat_threshold) of a tree: per categorical node, in node order, a bitset over category IDS of
    max member id // 32 + 1 words"""
    bounds, words = [0], []
    for n in sorted(t.cat):
        ids = [int(kept[t.feat[n]][b]) for b in t.cat[n]]
        w = [0] * (max(ids) // 32 + 1)
        for i in ids:
            w[i // 32] |= 1 << (i % 32)
        words += w
        bounds.append(len(words))
    return len(t.cat), bounds, words


def write_model(trees, cols, infos, lr, kept):
    head = ["tree", "version=v4", "num_class=1", "num_tree_per_iteration=1", "label_index=0", f"max_feature_idx={cols - 1}", "objective=lambdarank",
            "feature_names=" + " ".join(f"Column_{i}" for i in range(cols)), "feature_infos=" + " ".join(infos)]
    blocks = []
    ints = lambda a: " ".join(str(int(x)) for x in a)
    f64s = lambda a: " ".join(T.g17(x) for x in a)
    for i, t in enumerate(trees):
        nl = t.num_leaves
        num_cat, cb, ct = cat_lines(t, kept)
        b = [f"Tree={i}", f"num_leaves={nl}", f"num_cat={num_cat}", "split_feature=" + ints(t.feat),
             "split_gain=" + " ".join(format(float(np.float32(x)), ".9g") for x in t.gain), "threshold=" + f64s(t.thr), "decision_type=" + ints(t.dt),
             "left_child=" + ints(t.left), "right_child=" + ints(t.right), "leaf_value=" + f64s(t.value[l] for l in range(nl)),
             "leaf_weight=" + f64s(t.weight[l] for l in range(nl)), "leaf_count=" + ints(t.count[l] for l in range(nl)),
             "internal_value=" + f64s(t.ivalue), "internal_weight=" + f64s(t.iweight), "internal_count=" + ints(t.icount)]
        if num_cat:
            b += ["cat_boundaries=" + ints(cb), "cat_threshold=" + ints(ct)]
        b += ["is_linear=0", "shrinkage=" + T.g17(lr)]
        blocks.append("\n".join(b))
    head.append("tree_sizes=" + " ".join(str(len(b) + 3) for b in blocks))
    text = "\n".join(head) + "\n\n" + "".join(b + "\n\n\n" for b in blocks) + "end of trees\n\nfeature_importances:\n\nparameters:\n[boosting: gbdt]\n[objective: lambdarank]\n\nend of parameters\n\npandas_categorical:null\n"
    return text.encode("utf-8")


# ------------------------------------------------------------------ the fit
def fit(X, labels, offsets, valid=None, cfg=None, each=None):
    """train_reference.fit with cfg["categorical"] columns -> the same dict, plus kept (per column: the kept ids or None)"""
    cfg = parse_config(cfg)
    X = np.asarray(X, dtype=np.float64)
    rows, cols = X.shape
    if any(c >= cols for c in cfg["categorical"]):
        raise ValueError("categorical")
    is_cat = [c in cfg["categorical"] for c in range(cols)]
    y = np.asarray(labels, dtype=np.int64)
    offsets = [int(o) for o in offsets]
    max_bin = int(cfg["max_bin"])
    kept = [kept_categories(X[:, c], max_bin) if is_cat[c] else None for c in range(cols)]
    bounds = [np.zeros(0) if is_cat[c] else T.bin_bounds(X[:, c], max_bin) for c in range(cols)]
    nbins = [len(kept[c]) if is_cat[c] else len(bounds[c]) + 1 for c in range(cols)]
    bin_of = lambda M, c: bin_cat_column(M[:, c], kept[c]) if is_cat[c] else T.bin_column(M[:, c], bounds[c])
    binsT = [bin_of(X, c) for c in range(cols)]
    infos = [cat_feature_info(kept[c]) if is_cat[c] else T.feature_info(X[:, c]) for c in range(cols)]
    scores = np.zeros(rows, dtype=np.float64)
    if valid is not None:
        VX, vy, voff = np.asarray(valid[0], dtype=np.float64), np.asarray(valid[1], dtype=np.float64), [int(o) for o in valid[2]]
        vbinsT = [bin_of(VX, c) for c in range(cols)]
        vscores = np.zeros(len(vy), dtype=np.float64)
    trees, history = [], []
    best_it, best_metric, best_scores, best_vscores = 0, None, scores.copy(), None if valid is None else vscores.copy()
    for it in range(int(cfg["iterations"])):
        g, h = T.gradients(scores, y, offsets, float(cfg["sigma"]), int(cfg["truncation"]))
        gmax, hmax = float(np.max(np.abs(g))), float(np.max(h))
        if gmax == 0.0:
            break
        e_g, e_h = T.exponent(gmax, rows), T.exponent(hmax, rows)
        subset = T.feature_subset(cols, float(cfg["sampling"]), int(cfg["seed"]), it)
        t, leaf_of = grow_tree(binsT, nbins, is_cat, bounds, T.quantise(g, e_g), T.quantise(h, e_h), e_g, e_h, subset, cfg)
        if t is None:
            break
        trees.append(t)
        lv = np.array([t.value[l] for l in range(t.num_leaves)], dtype=np.float64)
        scores = scores + lv[leaf_of]
        if each is not None:
            each(it, g, h, t, scores)
        if valid is None:
            best_it, best_scores = len(trees), scores.copy()
            continue
        vscores = vscores + lv[route(t, vbinsT, len(vy))]
        m = E.mean(E.per_group(E.NDCG, int(cfg["ndcgCutoff"]), vscores, vy, voff, relpow=True, nolabels=1.0))
        history.append(m)
        if best_metric is None or m > best_metric:
            best_it, best_metric, best_scores, best_vscores = len(trees), m, scores.copy(), vscores.copy()
        elif len(trees) - best_it >= int(cfg["early_stopping"]):
            break
    return {"model": write_model(trees[:best_it], cols, infos, float(cfg["learningRate"]), kept), "iterations_run": len(trees), "best_iteration": best_it,
            "history": np.array(history, dtype=np.float64), "scores": best_scores, "valid_scores": best_vscores, "trees": trees, "kept": kept, "nbins": nbins}


# ------------------------------------------------------------------ data of the tests
MEMBERS = (1, 4, 7)


def dataset(seed, rows=1200, rare=True):
    """train_reference.dataset's 8 columns plus two categorical ones: column 8 holds ids 0 ... 9 (half of the cells with a fraction
    of 0.5: the id is the truncation) and, with `rare`, 3 + 2 + 1 cells of ids 20, 21, 22; column 9 holds ids 0 ... 2.  A row whose
    column 8 is in MEMBERS - no interval of the index order - gains two label steps, one whose column 9 is 1 gains one"""
    X, y, off = T.dataset(seed, rows=rows)
    rng = np.random.default_rng(1000 + seed)
    c8 = rng.integers(0, 10, rows).astype(np.float64)
    c9 = rng.integers(0, 3, rows).astype(np.float64)
    if rare:
        c8[rng.permutation(rows)[:6]] = [20, 20, 20, 21, 21, 22]
    y = np.clip(np.floor(0.5 * y) + 2.0 * np.isin(c8, MEMBERS) + (c9 == 1), 0, 4)
    c8 = c8 + 0.5 * (rng.random(rows) < 0.5)
    return np.column_stack([X, c8, c9]), y, off


def odd_cells(X, col, seed=0):
    """a copy of X whose column `col` holds, in four random rows each, NaN, a negative id, an id no training set here holds (77) and
    the rare id 22"""
    X = X.copy()
    idx = np.random.default_rng(seed).permutation(len(X))[:16]
    X[idx, col] = np.repeat([np.nan, -3.0, 77.0, 22.0], 4)
    return X, idx
