"""The xgboost backend's fit under tree_method "exact" with enable_categorical (include/mrk.h steps 2ec, 5ec) restated by
composing the two restatements that exist: a "q" column is searched by train_xgb_exact_reference (values, no bins), a "c" column is
binned and judged by train_xgb_cat_reference (kept ids, "other", the right sets); the highest gain wins, then the lowest column."""
import numpy as np

import train_reference as T
import train_xgb_cat_reference as TXC
import train_xgb_exact_reference as TXE
import train_xgb_reference as TX


def _goes_left(cells, bound, nan_left):
    """a "c" node carries its right set of bins where a "q" node carries its bound"""
    if isinstance(bound, tuple):
        return np.where(cells == TXC.NAN_BIN, bool(nan_left), ~np.isin(cells, bound))
    return _PLAIN_GOES_LEFT(cells, bound, nan_left)


def grow_tree(colsT, nbins, is_cat, bounds, qg, qh, e_g, e_h, sample, cfg):
    """TXE.grow_tree over colsT - f32 cells of a "q" column, bins of a "c" column - with both searches; t.cats as TXC.grow_tree's"""
    numeric = [np.zeros(len(qg), dtype=np.float32) if c else colsT[k] for k, c in enumerate(is_cat)]   # (a constant column has no candidate)

    def best_split(_, idx, sample, qg, qh, e_g, e_h, cfg):
        best = _PLAIN_BEST_SPLIT(numeric, idx, sample, qg, qh, e_g, e_h, cfg)
        for col in np.flatnonzero(is_cat):
            G, H, C = T._histogram(colsT, [col], idx[sample[idx]], qg, qh)
            c = TXC.best_cat_split(G[0], H[0], C[0], nbins[col], int(col), e_g, e_h, cfg)
            if c is not None and (best is None or c[0] > best[0] or (c[0] == best[0] and c[1] < best[1])):
                best = (c[0], c[1], 0, c[3], c[4], tuple(c[2]))
        return best

    TXE.best_split = best_split
    try:
        t, node_of = TXE.grow_tree(colsT, qg, qh, e_g, e_h, sample, cfg)
    finally:
        TXE.best_split = _PLAIN_BEST_SPLIT
    if t is not None:
        t.cats = {n: c for n, c in enumerate(t.cond) if isinstance(c, tuple)}
        for n in t.cats:
            t.cond[n] = np.float32(0.0)
    return t, node_of


def route(t, colsT, rows):
    cond = list(t.cond)
    for n, R in t.cats.items():
        t.cond[n] = R
    try:
        return TXE.route(t, colsT, rows)
    finally:
        t.cond = cond


_PLAIN_BEST_SPLIT, _PLAIN_GOES_LEFT = TXE.best_split, TXE.goes_left


def fit(X, labels, offsets, valid=None, cfg=None):
    """cfg as the device's: tree_method "exact", enable_categorical true, feature_types (position_bias too).  TXC.fit's loop, kept ids,
    bins of the "c" columns and model text; the f32 cells of TXE in the place of a "q" column's bins"""
    cfg = dict(cfg or {})
    assert cfg.pop("tree_method") == "exact" and cfg.pop("enable_categorical") is True
    plain = TX.bin_bounds, TX.bin_column, TXC.grow_tree, TXC.route
    TX.bin_bounds, TX.bin_column = (lambda column, max_bin=255: np.zeros(0)), (lambda column, bounds: TX.narrow(column) + np.float32(0.0))
    TXC.grow_tree, TXC.route, TXE.goes_left = grow_tree, route, _goes_left
    try:
        return TXC.fit(X, labels, offsets, valid=valid, cfg=cfg)
    finally:
        TX.bin_bounds, TX.bin_column, TXC.grow_tree, TXC.route = plain
        TXE.goes_left = _PLAIN_GOES_LEFT


def with_categories(X, y, ks, seed, nan_share=0.0):
    """X with one more "c" column per entry of ks - ids 0 ... k - 1 (the low ones frequent when k > 100) that move the label, a share of
    NaN that moves it too - and the feature_types"""
    rng = np.random.default_rng([seed, len(X)])
    ft = ["q"] * X.shape[1]
    for k in ks:
        ids = (k * rng.random(len(X)) ** (2.0 if k > 100 else 1.0)).astype(np.int64)
        col = ids + 0.25                                                       # (the category truncates)
        gone = rng.random(len(X)) < nan_share
        col[gone] = np.nan
        y = y + (rng.normal(size=k) * 1.5)[ids] * ~gone
        X, ft = np.column_stack([X, col]), ft + ["c"]
    return X, np.clip(np.floor(y), 0, 4), ft
