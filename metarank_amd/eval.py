"""Host-side mirror of the evaluation that ends the reference's `metarank train`.

Reference interfaces (ml/rank/LambdaMARTRanker.scala:115-123, :406-445):
    LambdaMARTModel.eval(dataset): scores every group of the test split with the booster, reduces it to the configured metric
    (NDCG(cutoff, nolabels = 1.0, relpow = true), default ndcg@10) and reports it beside noopArray and random scores.
`evaluate(booster, X, labels, group_offsets)` is that call; `eval_scores` takes scores the caller already has.  The sorting and
the ordered sums happen in libmrk_hip.so (csrc/eval.hip); there is no CPU path.  ltrlib's metric sources are not in the reference
tree: the formulas are include/mrk.h's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from .booster import Context, default_context

NDCG, MAP, MRR = 0, 1, 2
RELPOW = 1
METRICS = {"ndcg": NDCG, "map": MAP, "mrr": MRR}


def _metric(m) -> int:
    if isinstance(m, str):
        if m.lower() not in METRICS:
            raise N.MrkError(N.ERR_INVALID_ARG, f"unknown metric {m!r}")
        return METRICS[m.lower()]
    return int(m)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)


def _offsets(group_offsets):
    return np.ascontiguousarray(group_offsets, dtype=np.int64).reshape(-1)


def noop_array(group_offsets) -> np.ndarray:
    """noopArray (LambdaMARTRanker.scala:431-440) of every group back to back: (len - i) / len.toDouble"""
    off = _offsets(group_offsets)
    out = np.empty(int(off[-1]), dtype=np.float64)
    for lo, hi in zip(off[:-1], off[1:]):
        n = int(hi - lo)
        out[lo:hi] = (n - np.arange(n, dtype=np.float64)) / float(n)
    return out


def eval_scores(scores, labels, group_offsets, metric="ndcg", cutoff: int = 10, relpow: bool = True, nolabels: float = 1.0,
                per_group: bool = False, ctx: Context | None = None):
    """mrk_eval_scores: the mean of one metric over the groups (and, per_group, the value of every group)"""
    s, y, off = _f64(scores), _f64(labels), _offsets(group_offsets)
    n_groups = len(off) - 1
    rows = int(off[-1]) if n_groups >= 1 else 0
    if s.size != rows or y.size != rows:
        raise N.MrkError(N.ERR_INVALID_ARG, f"{s.size} scores / {y.size} labels, the offsets end at {rows}")
    ctx = ctx or default_context()
    value = C.c_double()
    groups = np.empty(max(n_groups, 1), dtype=np.float64) if per_group else None
    N.check(N.lib().mrk_eval_scores(ctx.handle, _metric(metric), int(cutoff), RELPOW if relpow else 0, float(nolabels), s.ctypes.data, y.ctypes.data,
                                    off.ctypes.data, n_groups, C.byref(value), None if groups is None else groups.ctypes.data))
    return (value.value, groups[:n_groups]) if per_group else value.value


def evaluate(booster, X, labels, group_offsets, metrics=(("ndcg", 10),), relpow: bool = True, nolabels: float = 1.0, seed=None,
             random_scores=None, return_scores: bool = False):
    """mrk_model_eval: per metric {"value", "noop", "random"}.  The random scores are numpy.random.default_rng(seed).random(rows)
    (the reference's are unseeded: only their role is reproduced) unless random_scores gives them."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise N.MrkError(N.ERR_INVALID_ARG, "X is not a matrix")
    y, off = _f64(labels), _offsets(group_offsets)
    n_groups = len(off) - 1
    rows, cols = X.shape
    if n_groups >= 1 and (int(off[-1]) != rows or y.size != rows):
        raise N.MrkError(N.ERR_INVALID_ARG, f"{rows} rows / {y.size} labels, the offsets end at {int(off[-1])}")
    metrics = list(metrics)
    ms = np.array([_metric(m) for m, _ in metrics], dtype=np.int32)
    ks = np.array([int(k) for _, k in metrics], dtype=np.int32)
    rnd = np.random.default_rng(seed).random(rows) if random_scores is None else _f64(random_scores)
    if rnd.size != rows:
        raise N.MrkError(N.ERR_INVALID_ARG, f"{rnd.size} random scores for {rows} rows")
    out = np.zeros((max(len(metrics), 1), 3), dtype=np.float64)
    scores = np.empty(rows, dtype=np.float64) if return_scores else None
    N.check(N.lib().mrk_model_eval(booster.handle, ms.ctypes.data, ks.ctypes.data, len(metrics), RELPOW if relpow else 0, float(nolabels), X.ctypes.data, cols,
                                   y.ctypes.data, off.ctypes.data, n_groups, rnd.ctypes.data, out.ctypes.data, None if scores is None else scores.ctypes.data))
    res = [{"value": float(v), "noop": float(n), "random": float(r)} for v, n, r in out[:len(metrics)]]
    return (res, scores) if return_scores else res


def labels_from_interactions(item_ids, interactions, weights) -> np.ndarray:
    """ClickthroughQuery.apply (lines 20-24), host-only: per item the FIRST interaction naming it decides - its `rel` if present,
    else weights.get(type, 0.0); an item without an interaction gets 0.0.  interactions: (item, type[, rel]) tuples or dicts
    with "item", "type" and optionally "rel"."""
    first = {}
    for it in interactions:
        if isinstance(it, dict):
            item, tpe, rel = it["item"], it.get("type"), it.get("rel")
        else:
            item, tpe, rel = it[0], it[1], (it[2] if len(it) > 2 else None)
        if item not in first:
            first[item] = float(rel) if rel is not None else float(weights.get(tpe, 0.0))
    return np.array([first.get(i, 0.0) for i in item_ids], dtype=np.float64)
