"""The LambdaMART fit of include/mrk.h (mrk_train_*) restated in Python / numpy.  The algorithm is this project's
(LightGBM's lambdarank objective and leaf-wise histogram learner where the rules are public, fixed-point sums and host-made tables
where a GPU needs them for bit-reproducibility); the GPU tests compare bit patterns and model bytes with these functions.

Order matters in exactly two places and both are loops here: an item adds its partners in ascending partner rank (group_gradients
loops over the partner rank q with a vector over the item rank r), and a tree's leaves are added to a score in tree order.  Every
sum over rows is an int64 sum of quantised values: numpy's summation order cannot change it.  exp and log2 are math.exp / math.log2:
the host's libm, as the library's tables."""
import math

import numpy as np

import eval_reference as E

SIGMOID_BINS = 65536
NAN_BIN = 255
MAX_GROUP = 4096
MASK64 = (1 << 64) - 1

DEFAULTS = {"iterations": 100, "learningRate": 0.1, "ndcgCutoff": 10, "maxDepth": 8, "seed": 0, "numLeaves": 16, "sampling": 0.8, "debias": False,
            "max_bin": 255, "truncation": 30, "sigma": 1.0, "min_data_in_leaf": 20, "min_sum_hessian": 1e-3, "lambda_l2": 0.0, "early_stopping": 20}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def parse_config(cfg=None):
    out = dict(DEFAULTS)
    for k, v in (cfg or {}).items():
        if k not in DEFAULTS:
            raise KeyError(k)
        if v is not None:
            out[k] = v
    return out


# ------------------------------------------------------------------ 2. bins
def bin_bounds(column, max_bin=255):
    """the upper bounds of a column's bins but the last; NaN cells are no values, -0.0 is +0.0"""
    v = np.asarray(column, dtype=np.float64)
    v = v[~np.isnan(v)]
    if np.isinf(v).any():
        raise ValueError("infinite cell")
    v = np.sort(v + 0.0)
    m = len(v)
    if m == 0:
        return np.zeros(0, dtype=np.float64)
    change = np.flatnonzero(v[1:] != v[:-1]) + 1          # p: v[p] != v[p - 1]
    if len(change) + 1 <= max_bin - 1:
        cuts = [int(p) for p in change]
    else:
        cuts = []
        for i in range(1, max_bin - 1):
            k = int(np.searchsorted(change, (i * m) // (max_bin - 1), side="left"))
            if k == len(change):
                break
            p = int(change[k])
            if not cuts or cuts[-1] != p:
                cuts.append(p)
    out = []
    for p in cuts:
        a, b = float(v[p - 1]), float(v[p])
        mid = (a + b) / 2.0
        if not mid < b:                                    # (also a sum that overflowed)
            mid = a
        out.append(mid)
    return np.array(out, dtype=np.float64)


def bin_column(column, bounds):
    x = np.asarray(column, dtype=np.float64)
    b = np.searchsorted(bounds, x, side="left").astype(np.int64)   # the number of bounds < x
    b[np.isnan(x)] = NAN_BIN
    return b.astype(np.uint8)


# ------------------------------------------------------------------ 7. feature subsets
def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & MASK64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return state, z ^ (z >> 31)


def feature_subset(cols, sampling, seed, tree):
    k = min(cols, max(1, int(math.floor(cols * sampling + 0.5))))
    state = ((seed & 0xffffffff) << 32) | (tree & 0xffffffff)
    idx = list(range(cols))
    for j in range(k):
        state, z = splitmix64(state)
        r = j + z % (cols - j)
        idx[j], idx[r] = idx[r], idx[j]
    return sorted(idx[:k])


# ------------------------------------------------------------------ 3. gradients
_tables = {}


def sigmoid_table(sigma):
    if sigma not in _tables:
        lo = -25.0 / sigma
        f = SIGMOID_BINS / (50.0 / sigma)
        _tables[sigma] = (lo, f, np.array([1.0 / (1.0 + math.exp(sigma * (lo + t / f))) for t in range(SIGMOID_BINS)], dtype=np.float64))
    return _tables[sigma]


def lg_tables(n):
    lg = np.array([math.log2(i + 2) for i in range(n)], dtype=np.float64)
    return lg, 1.0 / lg


def group_gradients(s, y, lg, invlg, sigma=1.0, truncation=30):
    """(g, h) of one group in item order; s: f64 scores, y: integer labels"""
    s = np.asarray(s, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    n = len(y)
    k = min(truncation, n)
    lo, f, T = sigmoid_table(sigma)
    sigma2 = sigma * sigma
    pi = np.array(E.order([float(v) for v in s]), dtype=np.int64)
    sr, yr = s[pi], y[pi]
    gain = np.ldexp(1.0, yr) - 1.0
    acc = 0.0
    for i, gn in enumerate(sorted((float(v) for v in gain), reverse=True)[:k]):
        acc = acc + gn / float(lg[i])
    inv = 0.0 if acc == 0.0 else 1.0 / acc
    r = np.arange(n)
    il = invlg[:n]
    g = np.zeros(n, dtype=np.float64)
    h = np.zeros(n, dtype=np.float64)
    for q in range(n):
        active = (yr != yr[q]) & ((r < k) | (q < k))
        if not active.any():
            continue
        r_hi = yr > yr[q]
        delta = np.where(r_hi, sr - sr[q], sr[q] - sr)
        rho = T[np.clip((delta - lo) * f, 0.0, SIGMOID_BINS - 1.0).astype(np.int64)]
        dg = np.where(r_hi, gain - gain[q], gain[q] - gain)
        w = (dg * np.abs(np.where(r_hi, il - il[q], il[q] - il))) * inv
        lam = (sigma * rho) * w
        eta = ((sigma2 * rho) * (1.0 - rho)) * w
        g = np.where(active, np.where(r_hi, g - lam, g + lam), g)
        h = np.where(active, h + eta, h)
    og, oh = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
    og[pi], oh[pi] = g, h
    return og, oh


def gradients(scores, labels, offsets, sigma=1.0, truncation=30):
    scores = np.asarray(scores, dtype=np.float64)
    labels = np.asarray(labels)
    lg, invlg = lg_tables(int(np.max(np.diff(offsets))))
    g, h = np.empty(len(scores), dtype=np.float64), np.empty(len(scores), dtype=np.float64)
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        g[lo:hi], h[lo:hi] = group_gradients(scores[lo:hi], labels[lo:hi], lg, invlg, sigma, truncation)
    return g, h


# ------------------------------------------------------------------ 4. quantise
def exponent(vmax, rows):
    return 0 if vmax == 0.0 else 61 - int(rows).bit_length() - math.frexp(vmax)[1]


def quantise(v, e):
    return np.rint(np.ldexp(v, e)).astype(np.int64)


def real(q, e):
    return np.ldexp(np.asarray(q, dtype=np.int64).astype(np.float64), -e)


# ------------------------------------------------------------------ 5. one tree
class Tree:
    """LightGBM's numbering: the s-th split makes internal node s, its left child keeps the leaf index, its right child is leaf s + 1"""

    def __init__(self):
        self.feat, self.gain, self.thr, self.dt, self.left, self.right = [], [], [], [], [], []
        self.bin, self.ivalue, self.iweight, self.icount = [], [], [], []
        self.parent = {0: None}      # leaf -> (node, side)
        self.depth = {0: 0}
        self.value, self.weight, self.count = {}, {}, {}

    @property
    def num_leaves(self):
        return len(self.feat) + 1

    def split(self, leaf, col, b, thr, nan_left, gain):
        s = len(self.feat)
        new = s + 1
        self.feat.append(col)
        self.bin.append(b)
        self.gain.append(gain)
        self.thr.append(thr)
        self.dt.append(8 | (2 if nan_left else 0))
        self.left.append(~leaf)
        self.right.append(~new)
        if self.parent[leaf] is not None:
            node, side = self.parent[leaf]
            (self.left if side == 0 else self.right)[node] = s
        self.parent[leaf], self.parent[new] = (s, 0), (s, 1)
        self.depth[leaf] = self.depth[new] = self.depth[leaf] + 1
        return new


def leaf_output(QG, QH, e_g, e_h, l2, lr):
    G, H = float(real(QG, e_g)), float(real(QH, e_h))
    return (-G / (H + l2)) * lr, H


def _histogram(binsT, subset, rows_idx, qg, qh):
    ns = len(subset)
    G, H, C = np.zeros((ns, 256), dtype=np.int64), np.zeros((ns, 256), dtype=np.int64), np.zeros((ns, 256), dtype=np.int64)
    for j, col in enumerate(subset):
        b = binsT[col][rows_idx]
        np.add.at(G[j], b, qg[rows_idx])
        np.add.at(H[j], b, qh[rows_idx])
        C[j] = np.bincount(b, minlength=256)
    return G, H, C


def _best_split(hist, subset, nbins, e_g, e_h, cfg):
    """(gain, col, b, nan_left, (QGL, QHL, CL)) of the best admitted candidate or None: the highest gain, then the lowest feature,
    the lowest bin, NaN to the right"""
    G, H, C = hist
    l2, mdl, msh = float(cfg["lambda_l2"]), int(cfg["min_data_in_leaf"]), float(cfg["min_sum_hessian"])
    best = None
    for j, col in enumerate(subset):
        nb = int(nbins[col])
        if nb < 2:
            continue
        cg, ch, cc = np.cumsum(G[j][:nb]), np.cumsum(H[j][:nb]), np.cumsum(C[j][:nb])
        ng, nh, nc = int(G[j][NAN_BIN]), int(H[j][NAN_BIN]), int(C[j][NAN_BIN])
        tg, th, tc = int(cg[-1]) + ng, int(ch[-1]) + nh, int(cc[-1]) + nc
        Gt, Ht = float(real(tg, e_g)), float(real(th, e_h))
        parent = (Gt * Gt) / (Ht + l2)
        for nan_left in ((0, 1) if nc > 0 else (0,)):
            QGL, QHL, CL = cg[:nb - 1] + nan_left * ng, ch[:nb - 1] + nan_left * nh, cc[:nb - 1] + nan_left * nc
            GL, HL, GR, HR = real(QGL, e_g), real(QHL, e_h), real(tg - QGL, e_g), real(th - QHL, e_h)
            with np.errstate(divide="ignore", invalid="ignore"):
                gain = ((GL * GL) / (HL + l2) + (GR * GR) / (HR + l2)) - parent
            ok = (CL >= mdl) & (tc - CL >= mdl) & (HL >= msh) & (HR >= msh) & (gain > 0.0)
            if not ok.any():
                continue
            gain = np.where(ok, gain, -np.inf)
            b = int(np.argmax(gain))                      # the first of equal gains: the lowest bin
            c = (float(gain[b]), col, b, nan_left, (int(QGL[b]), int(QHL[b]), int(CL[b])))
            # the highest gain, then the lowest column, then the lowest bin, then NaN to the right (columns and nan_left ascend here)
            if best is None or c[0] > best[0] or (c[0] == best[0] and col == best[1] and b < best[2]):
                best = c
    return best


def grow_tree(binsT, nbins, bounds, qg, qh, e_g, e_h, subset, cfg):
    """-> (Tree, leaf_of) or (None, None) when the root cannot split"""
    rows = len(qg)
    l2, lr = float(cfg["lambda_l2"]), float(cfg["learningRate"])
    leaf_of = np.zeros(rows, dtype=np.int64)
    t = Tree()
    totals = {0: (int(qg.sum()), int(qh.sum()), rows)}
    cand = {0: _best_split(_histogram(binsT, subset, np.arange(rows), qg, qh), subset, nbins, e_g, e_h, cfg)}
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
        v, w = leaf_output(tg, th, e_g, e_h, l2, lr)
        t.ivalue.append(v), t.iweight.append(w), t.icount.append(tc)
        new = t.split(leaf, col, b, float(bounds[col][b]), nan_left, gain)
        cb = binsT[col]
        goes_left = (cb <= b) | ((cb == NAN_BIN) & bool(nan_left))
        leaf_of[(leaf_of == leaf) & ~goes_left] = new
        totals[leaf], totals[new] = (QGL, QHL, CL), (tg - QGL, th - QHL, tc - CL)
        for lf in (leaf, new):
            idx = np.flatnonzero(leaf_of == lf)
            assert len(idx) == totals[lf][2]
            cand[lf] = _best_split(_histogram(binsT, subset, idx, qg, qh), subset, nbins, e_g, e_h, cfg) if t.depth[lf] < int(cfg["maxDepth"]) else None
    if t.num_leaves == 1:
        return None, None
    for lf in range(t.num_leaves):
        t.value[lf], t.weight[lf] = leaf_output(totals[lf][0], totals[lf][1], e_g, e_h, l2, lr)
        t.count[lf] = totals[lf][2]
    return t, leaf_of


def route(t, binsT, rows):
    """the leaf of every row of a binned matrix (the validation set's way through a new tree)"""
    out = np.empty(rows, dtype=np.int64)
    for i in range(rows):
        n = 0
        while n >= 0:
            b = int(binsT[t.feat[n]][i])
            left = (b <= t.bin[n]) or (b == NAN_BIN and (t.dt[n] & 2) != 0)
            n = t.left[n] if left else t.right[n]
        out[i] = ~n
    return out


# ------------------------------------------------------------------ the model text
def g17(x):
    return format(float(x), ".17g")


def feature_info(column):
    v = np.asarray(column, dtype=np.float64)
    v = v[~np.isnan(v)] + 0.0
    if len(v) == 0 or v.min() == v.max():
        return "none"
    return "[" + g17(v.min()) + ":" + g17(v.max()) + "]"


def write_model(trees, cols, infos, lr):
    head = ["tree", "version=v4", "num_class=1", "num_tree_per_iteration=1", "label_index=0", f"max_feature_idx={cols - 1}", "objective=lambdarank",
            "feature_names=" + " ".join(f"Column_{i}" for i in range(cols)), "feature_infos=" + " ".join(infos)]
    blocks = []
    for i, t in enumerate(trees):
        nl = t.num_leaves
        ints = lambda a: " ".join(str(int(x)) for x in a)
        f64s = lambda a: " ".join(g17(x) for x in a)
        b = [f"Tree={i}", f"num_leaves={nl}", "num_cat=0", "split_feature=" + ints(t.feat),
             "split_gain=" + " ".join(format(float(np.float32(x)), ".9g") for x in t.gain), "threshold=" + f64s(t.thr), "decision_type=" + ints(t.dt),
             "left_child=" + ints(t.left), "right_child=" + ints(t.right), "leaf_value=" + f64s(t.value[l] for l in range(nl)),
             "leaf_weight=" + f64s(t.weight[l] for l in range(nl)), "leaf_count=" + ints(t.count[l] for l in range(nl)),
             "internal_value=" + f64s(t.ivalue), "internal_weight=" + f64s(t.iweight), "internal_count=" + ints(t.icount), "is_linear=0", "shrinkage=" + g17(lr)]
        blocks.append("\n".join(b))
    head.append("tree_sizes=" + " ".join(str(len(b) + 3) for b in blocks))
    text = "\n".join(head) + "\n\n" + "".join(b + "\n\n\n" for b in blocks) + "end of trees\n\nfeature_importances:\n\nparameters:\n[boosting: gbdt]\n[objective: lambdarank]\n\nend of parameters\n\npandas_categorical:null\n"
    return text.encode("utf-8")


# ------------------------------------------------------------------ the fit
def fit(X, labels, offsets, valid=None, cfg=None, each=None):
    """-> dict(model, iterations_run, best_iteration, history, scores, valid_scores, trees).  valid: (X, labels, offsets)"""
    cfg = parse_config(cfg)
    X = np.asarray(X, dtype=np.float64)
    rows, cols = X.shape
    y = np.asarray(labels, dtype=np.int64)
    offsets = [int(o) for o in offsets]
    bounds = [bin_bounds(X[:, c], int(cfg["max_bin"])) for c in range(cols)]
    nbins = [len(b) + 1 for b in bounds]
    binsT = [bin_column(X[:, c], bounds[c]) for c in range(cols)]
    infos = [feature_info(X[:, c]) for c in range(cols)]
    scores = np.zeros(rows, dtype=np.float64)
    if valid is not None:
        VX, vy, voff = np.asarray(valid[0], dtype=np.float64), np.asarray(valid[1], dtype=np.float64), [int(o) for o in valid[2]]
        vbinsT = [bin_column(VX[:, c], bounds[c]) for c in range(cols)]
        vscores = np.zeros(len(vy), dtype=np.float64)
    trees, history = [], []
    best_it, best_metric, best_scores, best_vscores = 0, None, scores.copy(), None if valid is None else vscores.copy()
    for it in range(int(cfg["iterations"])):
        g, h = gradients(scores, y, offsets, float(cfg["sigma"]), int(cfg["truncation"]))
        gmax, hmax = float(np.max(np.abs(g))), float(np.max(h))
        if gmax == 0.0:
            break
        e_g, e_h = exponent(gmax, rows), exponent(hmax, rows)
        subset = feature_subset(cols, float(cfg["sampling"]), int(cfg["seed"]), it)
        t, leaf_of = grow_tree(binsT, nbins, bounds, quantise(g, e_g), quantise(h, e_h), e_g, e_h, subset, cfg)
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
    return {"model": write_model(trees[:best_it], cols, infos, float(cfg["learningRate"])), "iterations_run": len(trees), "best_iteration": best_it,
            "history": np.array(history, dtype=np.float64), "scores": best_scores, "valid_scores": best_vscores, "trees": trees}


# ------------------------------------------------------------------ data of the tests
def dataset(seed, rows=3000, lo=5, hi=40):
    """groups of lo ... hi rows (the last one cut so that exactly `rows` remain) x 8 columns: 0 constant, 1 with NaN, 2 with more
    than 255 distinct values, 3 with 4 distinct values, 4 and 5 copies of one column, 6 and 7 noise; labels 0 ... 4 follow columns 2 and 4"""
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < rows:
        sizes.append(int(rng.integers(lo, hi + 1)))
    sizes[-1] -= sum(sizes) - rows
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = rng.normal(size=(rows, 8))
    X[:, 0] = 3.0
    X[rng.random(rows) < 0.2, 1] = np.nan
    X[:, 3] = rng.integers(0, 4, rows)
    X[:, 5] = X[:, 4]
    y = np.clip(np.floor(X[:, 2] + X[:, 4] + rng.normal(size=rows) * 0.5 + 1.0), 0, 4)
    return X, y, off


def adjacent(seed, rows=1200):
    """dataset() whose column 3 holds prev(1.0), 1.0, next(1.0) and 2.0: the bound between 1.0 and its upper neighbour is 1.0 itself
    (no f64 lies between them), so cells sit AT a bound and one ulp on either side of it, and the labels make that bound the split to find"""
    X, y, off = dataset(seed, rows=rows)
    c3 = X[:, 3].astype(np.int64)
    X[:, 3] = np.array([np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), 2.0])[c3]
    return X, np.clip(y + 2.0 * (c3 >= 2), 0, 4), off


def learnable(seed, groups=400, n=20, noise=1.0):
    """the label is a monotone function of columns 0 and 1 plus noise; 6 columns"""
    rng = np.random.default_rng(seed)
    rows = groups * n
    X = rng.normal(size=(rows, 6))
    y = np.clip(np.floor(X[:, 0] + 0.5 * X[:, 1] + rng.normal(size=rows) * noise + 1.5), 0, 4)
    return X, y, np.arange(0, rows + 1, n, dtype=np.int64)
