"""The LambdaMART fit of the xgboost backend (include/mrk.h steps 2x, 5x, 6x, 7x) restated in Python / numpy.  Steps 1, 3,
4 and 8 are train_reference's and are imported from it.  What differs: bins are found and compared in f32 with the bound AT the upper
neighbour (x < bound goes left: the model's own test), a tree sees a sample of the ROWS and all columns, it grows level by level in
XGBoost's breadth-first numbering with every open node splitting on its own, scores are f32 sums from 0.5f, and the model text is
XGBoost's JSON.  The GPU tests compare bit patterns and model bytes with these functions; every sum over rows is an int64 sum."""
import numpy as np

import eval_reference as E
import train_reference as T

NAN_BIN = T.NAN_BIN
ROOT_PARENT = 2147483647
ROW_MUL = 0xD6E8FEB86659FD93

DEFAULTS = {"backend": "xgboost", "iterations": 100, "learningRate": 0.1, "ndcgCutoff": 10, "maxDepth": 8, "seed": 0, "sampling": 0.8, "debias": False,
            "max_bin": 255, "truncation": 30, "sigma": 1.0, "early_stopping": 20, "lambda": 1.0, "gamma": 0.0, "min_child_weight": 1.0, "categorical": []}
# keys of the default backend alone: refused by name (ValueError), where a key of no backend is unknown (KeyError)
LIGHTGBM_ONLY = ("numLeaves", "min_data_in_leaf", "min_sum_hessian", "lambda_l2", "max_cat_to_onehot", "max_cat_threshold", "cat_smooth", "cat_l2", "min_data_per_group")


def parse_config(cfg=None):
    out = dict(DEFAULTS)
    for k, v in (cfg or {}).items():
        if k not in DEFAULTS and k not in LIGHTGBM_ONLY:
            raise KeyError(k)
        if k in LIGHTGBM_ONLY and v is not None:
            raise ValueError(k + " is not a key of the xgboost backend")
        if v is not None:
            out[k] = v
    if out["backend"] != "xgboost" or not 1 <= int(out["maxDepth"]) <= 15 or not 0.0 < float(out["sampling"]) <= 1.0:
        raise ValueError("backend / maxDepth / sampling")
    if min(float(out["lambda"]), float(out["gamma"]), float(out["min_child_weight"])) < 0.0:
        raise ValueError("lambda / gamma / min_child_weight")
    if out["categorical"] or out["debias"]:
        raise NotImplementedError("categorical / debias")
    return out


# ------------------------------------------------------------------ 2x. bins
def narrow(column):
    """the cells as f32 (round to nearest even); a finite cell that becomes infinite, or an infinite one, is refused"""
    x = np.asarray(column, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)
    if np.isinf(f).any():
        raise ValueError("a cell that is not finite as an f32")
    return f


def bin_bounds(column, max_bin=255):
    """the bounds of a column's bins, f32 values widened to f64: the upper neighbour itself; bin(x) = the number of bounds <= (float) x"""
    f = narrow(column)
    v = np.sort(f[~np.isnan(f)] + np.float32(0.0))          # (-0.0f + 0.0f is +0.0f)
    m = len(v)
    if m == 0:
        return np.zeros(0, dtype=np.float64)
    change = np.flatnonzero(v[1:] != v[:-1]) + 1
    if len(change) + 1 <= max_bin - 1:
        cuts = [int(p) for p in change]
    else:                                                      # step 2's quantile walk, unchanged
        cuts = []
        for i in range(1, max_bin - 1):
            k = int(np.searchsorted(change, (i * m) // (max_bin - 1), side="left"))
            if k == len(change):
                break
            p = int(change[k])
            if not cuts or cuts[-1] != p:
                cuts.append(p)
    return np.array([float(v[p]) for p in cuts], dtype=np.float64)


def bin_column(column, bounds):
    f = narrow(column)
    b = np.searchsorted(bounds, f.astype(np.float64), side="right").astype(np.int64)   # the number of bounds <= x
    b[np.isnan(f)] = NAN_BIN
    return b.astype(np.uint8)


# ------------------------------------------------------------------ 7x. rows of a tree
def row_sampled(sampling, seed, tree, row):
    if sampling >= 1.0:
        return True
    state = ((((seed & 0xffffffff) << 32) | (tree & 0xffffffff)) ^ ((row * ROW_MUL) & T.MASK64)) & T.MASK64
    _, z = T.splitmix64(state)
    return (z >> 11) * 2.0 ** -53 < sampling


def row_sample(rows, sampling, seed, tree):
    return np.array([row_sampled(sampling, seed, tree, r) for r in range(rows)], dtype=bool)


# ------------------------------------------------------------------ 5x. one tree
class Tree:
    """XGBoost's arrays: node 0 is the root, a node that splits gives its children the next two free ids (breadth first)"""

    def __init__(self):
        self.left, self.right, self.parent, self.col, self.bin, self.default_left = [], [], [], [], [], []
        self.cond, self.base_weight, self.loss_change, self.sum_hessian = [], [], [], []
        self.depth = []

    @property
    def num_nodes(self):
        return len(self.left)

    @property
    def num_leaves(self):
        return sum(1 for l in self.left if l < 0)

    def add(self, parent, depth):
        self.left.append(-1), self.right.append(-1), self.parent.append(parent), self.col.append(0), self.bin.append(0), self.default_left.append(0)
        self.cond.append(np.float32(0.0)), self.base_weight.append(np.float32(0.0)), self.loss_change.append(np.float32(0.0)), self.sum_hessian.append(np.float32(0.0))
        self.depth.append(depth)
        return self.num_nodes - 1

    def weigh(self, node, QG, QH, e_g, e_h, lam, lr):
        G, H = float(T.real(QG, e_g)), float(T.real(QH, e_h))
        if H + lam == 0.0:
            raise ValueError("a node without a finite weight")
        w = -G / (H + lam)
        self.base_weight[node], self.sum_hessian[node] = np.float32(w), np.float32(H)
        if self.left[node] < 0:
            self.cond[node] = np.float32(w * lr)


def _best_split(hist, nbins, e_g, e_h, cfg):
    """train_reference._best_split under 5x's admission rule, over all columns"""
    G, H, C = hist
    lam, gamma, mcw = float(cfg["lambda"]), float(cfg["gamma"]), float(cfg["min_child_weight"])
    best = None
    for col in range(len(nbins)):
        nb = int(nbins[col])
        if nb < 2:
            continue
        cg, ch, cc = np.cumsum(G[col][:nb]), np.cumsum(H[col][:nb]), np.cumsum(C[col][:nb])
        ng, nh, nc = int(G[col][NAN_BIN]), int(H[col][NAN_BIN]), int(C[col][NAN_BIN])
        tg, th, tc = int(cg[-1]) + ng, int(ch[-1]) + nh, int(cc[-1]) + nc
        Gt, Ht = float(T.real(tg, e_g)), float(T.real(th, e_h))
        parent = (Gt * Gt) / (Ht + lam)
        for nan_left in ((0, 1) if nc > 0 else (0,)):
            QGL, QHL, CL = cg[:nb - 1] + nan_left * ng, ch[:nb - 1] + nan_left * nh, cc[:nb - 1] + nan_left * nc
            GL, HL, GR, HR = T.real(QGL, e_g), T.real(QHL, e_h), T.real(tg - QGL, e_g), T.real(th - QHL, e_h)
            with np.errstate(divide="ignore", invalid="ignore"):
                gain = ((GL * GL) / (HL + lam) + (GR * GR) / (HR + lam)) - parent
            ok = (CL >= 1) & (tc - CL >= 1) & (HL >= mcw) & (HR >= mcw) & (gain > gamma)
            if not ok.any():
                continue
            gain = np.where(ok, gain, -np.inf)
            b = int(np.argmax(gain))
            c = (float(gain[b]), col, b, nan_left, (int(QGL[b]), int(QHL[b]), int(CL[b])))
            if best is None or c[0] > best[0] or (c[0] == best[0] and col == best[1] and b < best[2]):
                best = c
    return best


def grow_tree(binsT, nbins, bounds, qg, qh, e_g, e_h, sample, cfg):
    """-> (Tree, node_of) or (None, None) when the root cannot split.  Level by level; EVERY open node with an admitted candidate
    splits.  A histogram holds the sampled rows only; every row is routed."""
    rows, cols = len(qg), len(nbins)
    lam, lr, max_depth = float(cfg["lambda"]), float(cfg["learningRate"]), int(cfg["maxDepth"])
    node_of = np.zeros(rows, dtype=np.int64)
    t = Tree()
    t.add(ROOT_PARENT, 0)
    totals = {0: (int(qg[sample].sum()), int(qh[sample].sum()), int(sample.sum()))}
    level = [0]
    d = 0
    while level:
        nxt = []
        for node in level:                                    # ascending id
            best = None
            if d < max_depth and totals[node][2] >= 2:
                idx = np.flatnonzero((node_of == node) & sample)
                assert len(idx) == totals[node][2]
                best = _best_split(T._histogram(binsT, list(range(cols)), idx, qg, qh), nbins, e_g, e_h, cfg)
            if best is None:
                continue
            gain, col, b, nan_left, (QGL, QHL, CL) = best
            tg, th, tc = totals[node]
            t.col[node], t.bin[node], t.default_left[node] = col, b, nan_left
            t.cond[node], t.loss_change[node] = np.float32(bounds[col][b]), np.float32(gain)
            l, r = t.add(node, d + 1), t.add(node, d + 1)
            t.left[node], t.right[node] = l, r
            cb = binsT[col]
            mine = node_of == node
            goes_left = (cb <= b) | ((cb == NAN_BIN) & bool(nan_left))
            node_of[mine & goes_left] = l
            node_of[mine & ~goes_left] = r
            totals[l], totals[r] = (QGL, QHL, CL), (tg - QGL, th - QHL, tc - CL)
            nxt += [l, r]
        level = nxt
        d += 1
    if t.num_nodes == 1:
        return None, None
    for node in range(t.num_nodes):
        t.weigh(node, totals[node][0], totals[node][1], e_g, e_h, lam, lr)
    return t, node_of


def route(t, binsT, rows):
    out = np.empty(rows, dtype=np.int64)
    for i in range(rows):
        n = 0
        while t.left[n] >= 0:
            b = int(binsT[t.col[n]][i])
            left = (b <= t.bin[n]) or (b == NAN_BIN and t.default_left[n] != 0)
            n = t.left[n] if left else t.right[n]
        out[i] = n
    return out


# ------------------------------------------------------------------ the model text
def g9(x):
    return "%.9g" % float(np.float32(x))


def write_model(trees, cols):
    """workloads/synth.py xgboost_document's shape and key order, no whitespace, every f32 as %.9g of its widened value"""
    ints = lambda key, a: '"%s":[%s],' % (key, ",".join(str(int(x)) for x in a))
    f32s = lambda key, a: '"%s":[%s],' % (key, ",".join(g9(x) for x in a))
    blocks = []
    for i, t in enumerate(trees):
        n = t.num_nodes
        blocks.append("{" + f32s("base_weights", t.base_weight) + '"categories":[],"categories_nodes":[],"categories_segments":[],"categories_sizes":[],' +
                      ints("default_left", t.default_left) + '"id":%d,' % i + ints("left_children", t.left) + f32s("loss_changes", t.loss_change) +
                      ints("parents", t.parent) + ints("right_children", t.right) + f32s("split_conditions", t.cond) + ints("split_indices", t.col) +
                      ints("split_type", [0] * n) + f32s("sum_hessian", t.sum_hessian) +
                      '"tree_param":{"num_deleted":"0","num_feature":"%d","num_nodes":"%d","size_leaf_vector":"1"}}' % (cols, n))
    nt = len(trees)
    text = ('{"learner":{"attributes":{},"feature_names":[],"feature_types":[],"gradient_booster":{"model":{"gbtree_model_param":{"num_parallel_tree":"1","num_trees":"%d"},'
            '"iteration_indptr":[%s],"tree_info":[%s],"trees":[%s]},"name":"gbtree"},"learner_model_param":{"base_score":"5E-1","boost_from_average":"1","num_class":"0",'
            '"num_feature":"%d","num_target":"1"},"objective":{"name":"rank:ndcg","lambdarank_param":{}}},"version":[2,1,0]}'
            % (nt, ",".join(str(i) for i in range(nt + 1)), ",".join("0" for _ in range(nt)), ",".join(blocks), cols))
    return text.encode("utf-8")


# ------------------------------------------------------------------ the fit
def fit(X, labels, offsets, valid=None, cfg=None, each=None):
    """-> dict(model, iterations_run, best_iteration, history, scores, valid_scores, trees, samples).  valid: (X, labels, offsets)"""
    cfg = parse_config(cfg)
    X = np.asarray(X, dtype=np.float64)
    rows, cols = X.shape
    y = np.asarray(labels, dtype=np.int64)
    offsets = [int(o) for o in offsets]
    bounds = [bin_bounds(X[:, c], int(cfg["max_bin"])) for c in range(cols)]
    nbins = [len(b) + 1 for b in bounds]
    binsT = [bin_column(X[:, c], bounds[c]) for c in range(cols)]
    scores = np.full(rows, 0.5, dtype=np.float32)                                  # 6x: f32 from the base_score
    if valid is not None:
        VX, vy, voff = np.asarray(valid[0], dtype=np.float64), np.asarray(valid[1], dtype=np.float64), [int(o) for o in valid[2]]
        vbinsT = [bin_column(VX[:, c], bounds[c]) for c in range(cols)]
        vscores = np.full(len(vy), 0.5, dtype=np.float32)
    trees, history, samples = [], [], []
    best_it, best_metric, best_scores, best_vscores = 0, None, scores.copy(), None if valid is None else vscores.copy()
    for it in range(int(cfg["iterations"])):
        g, h = T.gradients(scores.astype(np.float64), y, offsets, float(cfg["sigma"]), int(cfg["truncation"]))
        gmax, hmax = float(np.max(np.abs(g))), float(np.max(h))
        if gmax == 0.0:
            break
        e_g, e_h = T.exponent(gmax, rows), T.exponent(hmax, rows)
        sample = row_sample(rows, float(cfg["sampling"]), int(cfg["seed"]), it)
        t, node_of = grow_tree(binsT, nbins, bounds, T.quantise(g, e_g), T.quantise(h, e_h), e_g, e_h, sample, cfg)
        if t is None:
            break
        trees.append(t)
        samples.append(sample)
        lv = np.array(t.cond, dtype=np.float32)
        scores = scores + lv[node_of]                                               # f32 + f32, one rounding
        if each is not None:
            each(it, g, h, t, scores)
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
    return {"model": write_model(trees[:best_it], cols), "iterations_run": len(trees), "best_iteration": best_it, "history": np.array(history, dtype=np.float64),
            "scores": best_scores.astype(np.float64), "valid_scores": None if valid is None else best_vscores.astype(np.float64), "trees": trees, "samples": samples,
            "bounds": bounds}


def adjacent(seed, rows=1200):
    """T.dataset whose column 3 holds prev32(1), 1, next32(1) and 2 - and, in place of some of the 1s, f64 cells such as 1 + 1e-12 and
    1 - 1e-12 that narrow to exactly 1.0f (f64-side binning puts them on the wrong side of a bound at 1 or beside it); the labels make
    the bound at next32(1) the split to find"""
    X, y, off = T.dataset(seed, rows=rows)
    c3 = X[:, 3].astype(np.int64)
    one = np.float32(1.0)
    vals = np.array([float(np.nextafter(one, np.float32(0.0))), 1.0, float(np.nextafter(one, np.float32(2.0))), 2.0])
    col = vals[c3]
    ones = np.flatnonzero(c3 == 1)
    col[ones[0::3]] = 1.0 + 1e-12
    col[ones[1::3]] = 1.0 - 1e-12
    X[:, 3] = col
    return X, np.clip(y + 2.0 * (c3 >= 2), 0, 4), off
