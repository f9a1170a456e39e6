"""Step 3b of include/mrk.h (position_bias: Unbiased LambdaMART's correction) restated in Python / numpy.  Everything else
of a fit is train_reference's or train_xgb_reference's: `fit` runs THEIR boosting loop with the gradient step replaced.  An item adds
its pairs in ascending partner rank (the loop over q), every sum over rows is an int64 sum, exp / log1p / pow are math's."""
import math

import numpy as np

import eval_reference as E
import train_reference as T
import train_xgb_reference as TX

_cost = {}


def cost_table(sigma):
    if sigma not in _cost:
        lo, f, _ = T.sigmoid_table(sigma)
        _cost[sigma] = np.array([math.log1p(math.exp(-sigma * (lo + t / f))) for t in range(T.SIGMOID_BINS)], dtype=np.float64)
    return _cost[sigma]


def group_gradients(s, y, lg, invlg, tp, tm, sigma=1.0, truncation=30):
    """(g, h, cp, cm) of one group in item order: T.group_gradients with every pair divided by c = t_plus[pos(hi)] * t_minus[pos(lo)]"""
    s, y = np.asarray(s, dtype=np.float64), np.asarray(y, dtype=np.int64)
    n = len(y)
    k = min(truncation, n)
    lo, f, Tab = T.sigmoid_table(sigma)
    L = cost_table(sigma)
    sigma2 = sigma * sigma
    pi = np.array(E.order([float(v) for v in s]), dtype=np.int64)
    sr, yr = s[pi], y[pi]
    pos = np.minimum(pi, len(tp) - 1)                        # the place in the list as shown of the item at each rank
    gain = np.ldexp(1.0, yr) - 1.0
    acc = 0.0
    for i, gn in enumerate(sorted((float(v) for v in gain), reverse=True)[:k]):
        acc = acc + gn / float(lg[i])
    inv = 0.0 if acc == 0.0 else 1.0 / acc
    r, il = np.arange(n), invlg[:n]
    g, h, cp, cm = (np.zeros(n, dtype=np.float64) for _ in range(4))
    for q in range(n):
        active = (yr != yr[q]) & ((r < k) | (q < k))
        if not active.any():
            continue
        r_hi = yr > yr[q]
        delta = np.where(r_hi, sr - sr[q], sr[q] - sr)
        t = np.clip((delta - lo) * f, 0.0, T.SIGMOID_BINS - 1.0).astype(np.int64)
        rho = Tab[t]
        dg = np.where(r_hi, gain - gain[q], gain[q] - gain)
        w = (dg * np.abs(np.where(r_hi, il - il[q], il[q] - il))) * inv
        x = np.where(r_hi, tm[pos[q]], tp[pos[q]])           # the partner's factor
        c = np.where(r_hi, tp[pos], tm[pos]) * x
        lam = ((sigma * rho) * w) / c
        eta = (((sigma2 * rho) * (1.0 - rho)) * w) / c
        share = (L[t] * w) / x
        g = np.where(active, np.where(r_hi, g - lam, g + lam), g)
        h = np.where(active, h + eta, h)
        cp = np.where(active & r_hi, cp + share, cp)
        cm = np.where(active & ~r_hi, cm + share, cm)
    out = [np.empty(n, dtype=np.float64) for _ in range(4)]
    for o, v in zip(out, (g, h, cp, cm)):
        o[pi] = v
    return out


def gradients(scores, labels, offsets, tp, tm, sigma=1.0, truncation=30):
    scores, labels = np.asarray(scores, dtype=np.float64), np.asarray(labels)
    tp, tm = np.asarray(tp, dtype=np.float64), np.asarray(tm, dtype=np.float64)
    lg, invlg = T.lg_tables(int(np.max(np.diff(offsets))))
    out = [np.empty(len(scores), dtype=np.float64) for _ in range(4)]
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        for o, v in zip(out, group_gradients(scores[lo:hi], labels[lo:hi], lg, invlg, tp, tm, sigma, truncation)):
            o[lo:hi] = v
    return out


def position_sums(cost, offsets, positions):
    """(Q, e): the int64 sum of the quantised costs per position, under step 4's exponent rule"""
    off = np.asarray(offsets, dtype=np.int64)
    e = T.exponent(float(np.max(cost)), len(cost))
    pos = np.minimum(np.arange(len(cost)) - np.repeat(off[:-1], np.diff(off)), positions - 1)
    Q = np.zeros(positions, dtype=np.int64)
    np.add.at(Q, pos, T.quantise(cost, e))
    return Q, e


def update(t, Q, e, norm):
    S = T.real(Q, e)
    if S[0] == 0.0:
        return t
    out = t.copy()
    for i in range(len(t)):
        if S[i] > 0.0:
            out[i] = math.pow(float(S[i]) / float(S[0]), 1.0 / (norm + 1.0))
    return out


def fit(X, labels, offsets, valid=None, cfg=None):
    """the backend's restated fit with step 3b in place of step 3; adds t_plus, t_minus and sums (Qp, Qm per iteration) to its dict"""
    cfg = dict(cfg or {})
    pb = cfg.pop("position_bias", None)
    ref = TX if cfg.get("backend") == "xgboost" else T
    if pb is None:
        return ref.fit(X, labels, offsets, valid=valid, cfg=cfg)
    P, norm = pb.get("positions") or 32, 1.0 if pb.get("norm") is None else float(pb["norm"])
    state = {"tp": np.ones(P), "tm": np.ones(P), "sums": []}

    def biased(scores, labels, offsets, sigma=1.0, truncation=30):
        g, h, cp, cm = gradients(scores, labels, offsets, state["tp"], state["tm"], sigma, truncation)
        (Qp, ep), (Qm, em) = position_sums(cp, offsets, P), position_sums(cm, offsets, P)
        state["tp"], state["tm"] = update(state["tp"], Qp, ep, norm), update(state["tm"], Qm, em, norm)
        state["sums"].append((Qp, Qm))
        return g, h

    plain, T.gradients = T.gradients, biased                  # (both restated loops find their gradient step in train_reference)
    try:
        out = ref.fit(X, labels, offsets, valid=valid, cfg=cfg)
    finally:
        T.gradients = plain
    out["t_plus"], out["t_minus"], out["sums"] = state["tp"], state["tm"], state["sums"]
    return out
