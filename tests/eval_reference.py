"""The arithmetic of the ranking evaluation (include/mrk.h) restated in plain Python: loops, math.log2, math.pow.
The GPU tests compare bit patterns with these functions; `evaluate_numpy` is a vectorised form of the same quantities that only
tools/eval_bench.py times (numpy's pairwise sums are not the sequential ones: it is no oracle).

Pinned by the reference tree: NDCG(cutoff, nolabels = 1.0, relpow = true), noopArray(len)(i) = (len - i) / len.toDouble, the mean
over groups.  Everything else is this project's reading of ltrlib's metrics, whose sources the tree does not hold."""
import math
import struct

import numpy as np

NDCG, MAP, MRR = 0, 1, 2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def sort_key(score: float) -> int:
    """csrc/sort_device.hpp: the unsigned key whose integer order is java.lang.Double.compare's order of -score"""
    v = -score
    b = 0x7ff8000000000000 if v != v else struct.unpack("<Q", struct.pack("<d", v))[0]
    return (~b & 0xffffffffffffffff) if b & 0x8000000000000000 else (b | 0x8000000000000000)


def order(scores):
    """pi: sortBy(-score) - NaN last, +0.0 before -0.0, ties in group order"""
    return sorted(range(len(scores)), key=lambda i: (sort_key(float(scores[i])), i))


def gain(y: float, relpow: bool) -> float:
    return math.pow(2.0, y) - 1.0 if relpow else y


def _dcg(gains, k):
    s = None
    for i in range(k):
        t = gains[i] / math.log2(i + 2)
        s = t if s is None else s + t
    return s


def ndcg(scores, labels, cutoff=0, relpow=True, nolabels=1.0, pi=None):
    n = len(labels)
    k = n if cutoff == 0 else min(cutoff, n)
    pi = order(scores) if pi is None else pi
    g = [gain(float(y), relpow) for y in labels]
    ideal = [g[i] for i in order(g)]          # the gains sorted descending
    idcg = _dcg(ideal, k)
    if idcg == 0.0:
        return nolabels
    return _dcg([g[i] for i in pi], k) / idcg


def average_precision(scores, labels, cutoff=0, pi=None):
    n = len(labels)
    k = n if cutoff == 0 else min(cutoff, n)
    pi = order(scores) if pi is None else pi
    R = sum(1 for y in labels if y > 0)
    if R == 0:
        return 0.0
    hits, s = 0, 0.0
    for i in range(k):
        if labels[pi[i]] > 0:
            hits += 1
            s = s + float(hits) / float(i + 1)
    return s / float(min(R, k))


def reciprocal_rank(scores, labels, pi=None):
    pi = order(scores) if pi is None else pi
    for r, i in enumerate(pi, 1):
        if labels[i] > 0:
            return 1.0 / float(r)
    return 0.0


def group_value(metric, cutoff, scores, labels, relpow=True, nolabels=1.0, pi=None):
    if metric == NDCG:
        return ndcg(scores, labels, cutoff, relpow, nolabels, pi)
    if metric == MAP:
        return average_precision(scores, labels, cutoff, pi)
    return reciprocal_rank(scores, labels, pi)


def orders(scores, offsets):
    """pi of every group (computed once where several metrics are asked of the same scores)"""
    return [order([float(v) for v in scores[lo:hi]]) for lo, hi in zip(offsets[:-1], offsets[1:])]


def per_group(metric, cutoff, scores, labels, offsets, relpow=True, nolabels=1.0, noop=False, pis=None):
    """the value of every group; noop: pi is the identity (noopArray is strictly decreasing); pis: orders(scores, offsets)"""
    out = []
    for j, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
        y = [float(v) for v in labels[lo:hi]]
        if noop:
            s, pi = None, list(range(hi - lo))
        elif pis is not None:
            s, pi = None, pis[j]
        else:
            s, pi = [float(v) for v in scores[lo:hi]], None
        out.append(group_value(metric, cutoff, s, y, relpow, nolabels, pi))
    return np.array(out, dtype=np.float64)


def mean(values) -> float:
    s = None
    for v in values:
        s = float(v) if s is None else s + float(v)
    return s / float(len(values))


def noop_array(offsets):
    out = []
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        n = int(hi - lo)
        out += [(n - i) / float(n) for i in range(n)]
    return np.array(out, dtype=np.float64)


def evaluate_numpy(scores, labels, offsets, cutoff=10, relpow=True, nolabels=1.0):
    """ndcg@cutoff of every group, vectorised per group (tools/eval_bench.py's host comparison; not bit-exact with the loops)"""
    lg = np.log2(np.arange(2, int(np.max(np.diff(offsets))) + 2, dtype=np.float64))
    g_all = np.power(2.0, labels) - 1.0 if relpow else np.asarray(labels, dtype=np.float64)
    out = np.empty(len(offsets) - 1, dtype=np.float64)
    for j in range(len(out)):
        lo, hi = offsets[j], offsets[j + 1]
        g = g_all[lo:hi]
        k = hi - lo if cutoff == 0 else min(cutoff, hi - lo)
        top = np.argsort(-scores[lo:hi], kind="stable")[:k]
        idcg = float(np.sum(np.sort(g)[::-1][:k] / lg[:k]))
        out[j] = nolabels if idcg == 0.0 else float(np.sum(g[top] / lg[:k])) / idcg
    return out
