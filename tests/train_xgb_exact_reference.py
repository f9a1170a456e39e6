"""The xgboost backend's fit under tree_method "exact" (include/mrk.h steps 2e, 5e) restated in Python / numpy: no bins.
Everything but the split search and the routing by x < bound is train_xgb_reference's / train_reference's - its fit loop included.
Kept plain on purpose - per node and column one sort and one cumulative sum - so that it states the result, not the kernels."""
import numpy as np

import train_reference as T
import train_xgb_reference as TX


def parse_config(cfg=None):
    cfg = dict(cfg or {})
    method = cfg.pop("tree_method", None) or "hist"
    if method not in ("hist", "exact"):
        raise ValueError("tree_method = %r (hist or exact)" % method)
    return dict(TX.parse_config(cfg), tree_method=method)


def cells(X):
    """2e: per column the cells narrowed to f32, -0.0f as +0.0f"""
    return [TX.narrow(X[:, c]) + np.float32(0.0) for c in range(X.shape[1])]


def best_split(cols32, idx, sample, qg, qh, e_g, e_h, cfg):
    """5e at one node (idx: its rows, ascending): (gain, col, position, nan_left, (QGL, QHL, CL), bound) of the best admitted candidate
    or None.  A candidate stands between two neighbouring distinct non-NaN values of the node's rows, sampled or not; the sums and the
    counts are the sampled rows'.  The highest gain, then the lowest column, the lowest position, NaN right"""
    lam, gamma, mcw = float(cfg["lambda"]), float(cfg["gamma"]), float(cfg["min_child_weight"])
    s = sample[idx]
    tg, th, tc = int(qg[idx][s].sum()), int(qh[idx][s].sum()), int(s.sum())
    Gt, Ht = float(T.real(tg, e_g)), float(T.real(th, e_h))
    parent = (Gt * Gt) / (Ht + lam)
    best = None
    for col, cells32 in enumerate(cols32):
        order = np.lexsort((idx, cells32[idx]))                   # by (value, row), NaN last
        rows, v = idx[order], cells32[idx][order]
        sm = sample[rows]
        cg, ch, cc = np.cumsum(np.where(sm, qg[rows], 0)), np.cumsum(np.where(sm, qh[rows], 0)), np.cumsum(sm.astype(np.int64))
        nan = np.isnan(v)
        at = np.flatnonzero(~nan[:-1] & ~nan[1:] & (v[:-1] != v[1:]))   # the rows up to `at` go left
        if len(at) == 0:
            continue
        m = int((~nan).sum())
        ng, nh, nc = int(cg[-1] - cg[m - 1]), int(ch[-1] - ch[m - 1]), int(cc[-1] - cc[m - 1])
        for nan_left in ((0, 1) if nc > 0 else (0,)):
            QGL, QHL, CL = cg[at] + nan_left * ng, ch[at] + nan_left * nh, cc[at] + nan_left * nc
            GL, HL, GR, HR = T.real(QGL, e_g), T.real(QHL, e_h), T.real(tg - QGL, e_g), T.real(th - QHL, e_h)
            with np.errstate(divide="ignore", invalid="ignore"):
                gain = ((GL * GL) / (HL + lam) + (GR * GR) / (HR + lam)) - parent
            ok = (CL >= 1) & (tc - CL >= 1) & (HL >= mcw) & (HR >= mcw) & (gain > gamma)
            if not ok.any():
                continue
            gain = np.where(ok, gain, -np.inf)
            b = int(np.argmax(gain))
            c = (float(gain[b]), col, int(at[b]), nan_left, (int(QGL[b]), int(QHL[b]), int(CL[b])), np.float32(v[at[b] + 1]))
            if best is None or c[0] > best[0] or (c[0] == best[0] and col == best[1] and c[2] < best[2]):
                best = c
    return best


def goes_left(x32, bound, nan_left):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x32), bool(nan_left), x32 < bound)


def grow_tree(cols32, qg, qh, e_g, e_h, sample, cfg):
    """train_xgb_reference.grow_tree with 5e's search: -> (Tree, node_of) or (None, None) when the root cannot split"""
    lam, lr, max_depth = float(cfg["lambda"]), float(cfg["learningRate"]), int(cfg["maxDepth"])
    node_of = np.zeros(len(qg), dtype=np.int64)
    t = TX.Tree()
    t.add(TX.ROOT_PARENT, 0)
    totals = {0: (int(qg[sample].sum()), int(qh[sample].sum()), int(sample.sum()))}
    level, d = [0], 0
    while level:
        nxt = []
        for node in level:                                        # ascending id
            idx = np.flatnonzero(node_of == node)
            best = best_split(cols32, idx, sample, qg, qh, e_g, e_h, cfg) if d < max_depth else None
            if best is None:
                continue
            gain, col, _, nan_left, (QGL, QHL, CL), bound = best
            tg, th, tc = totals[node]
            t.col[node], t.default_left[node], t.cond[node], t.loss_change[node] = col, nan_left, bound, np.float32(gain)
            l, r = t.add(node, d + 1), t.add(node, d + 1)
            t.left[node], t.right[node] = l, r
            node_of[idx] = np.where(goes_left(cols32[col][idx], bound, nan_left), l, r)
            totals[l], totals[r] = (QGL, QHL, CL), (tg - QGL, th - QHL, tc - CL)
            nxt += [l, r]
        level = nxt
        d += 1
    if t.num_nodes == 1:
        return None, None
    for node in range(t.num_nodes):
        t.weigh(node, totals[node][0], totals[node][1], e_g, e_h, lam, lr)
    return t, node_of


def route(t, cols32, rows):
    """every row's leaf under the model's own test: (float) x < split_condition, NaN by default_left"""
    node = np.zeros(rows, dtype=np.int64)
    for n in range(t.num_nodes):                                  # (a child's id is above its parent's)
        if t.left[n] < 0:
            continue
        here = np.flatnonzero(node == n)
        node[here] = np.where(goes_left(cols32[t.col[n]][here], t.cond[n], t.default_left[n]), t.left[n], t.right[n])
    return node


_HIST_FIT = TX.fit


def fit(X, labels, offsets, valid=None, cfg=None):
    """train_xgb_reference.fit's loop and dict with 2e / 5e in the places of its bins, its search and its routing; tree_method "hist"
    (or none) IS train_xgb_reference.fit"""
    cfg = parse_config(cfg)
    if cfg.pop("tree_method") == "hist":
        return _HIST_FIT(X, labels, offsets, valid=valid, cfg=cfg)
    plain = TX.bin_bounds, TX.bin_column, TX.grow_tree, TX.route
    TX.bin_bounds, TX.bin_column, TX.route = (lambda column, max_bin=255: np.zeros(0)), (lambda column, bounds: TX.narrow(column) + np.float32(0.0)), route
    TX.grow_tree = lambda cols32, nbins, bounds, qg, qh, e_g, e_h, sample, cfg: grow_tree(cols32, qg, qh, e_g, e_h, sample, cfg)
    try:
        return _HIST_FIT(X, labels, offsets, valid=valid, cfg=cfg)
    finally:
        TX.bin_bounds, TX.bin_column, TX.grow_tree, TX.route = plain


def coarse(X, levels=6):
    """X with every column cut to at most `levels` + 1 distinct values (NaN kept): what `hist` bins without loss"""
    with np.errstate(invalid="ignore"):
        return np.clip(np.round(np.asarray(X, dtype=np.float64) * (levels / 6.0)), -(levels // 2), levels // 2)
