"""GPU: step 3b of the LambdaMART fits (position_bias; csrc/train.hip's biased LambdaRank kernels and the position-sum kernel) against its
restatement (tests/train_bias_reference.py): bit patterns and model bytes, no tolerances."""
import numpy as np
import pytest

import train_bias_reference as TB
import train_reference as T
import metarank_amd as M
from metarank_amd.train import fit_lambdamart, lambdarank_gradients

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def same_bits(got, want, what):
    a, b = T.bits(got), T.bits(want)
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {len(a)} differ, first at {int(np.flatnonzero(a != b)[0])}"


# n: 64 | 65 is the wavefront / workgroup kernel boundary; P < n clamps, P > n leaves factors unused; (1100, 1100) reads factors beyond
# the 1024 per side that the workgroup kernel stages in LDS
@pytest.mark.parametrize("n,P", [(n, P) for n in (1, 2, 63, 64, 65, 200) for P in (1, 4, 64)] + [(1100, 1100)])
def test_biased_gradients_against_the_restatement(ctx, n, P):
    rng = np.random.default_rng(1000 * n + P)
    groups = 6 if n <= 200 else 2                              # (six: two workgroups of the wavefront kernel)
    rows, last = groups * n, (groups - 1) * n
    off = np.arange(0, rows + 1, n, dtype=np.int64)
    scores = np.round(rng.normal(size=rows), 1)                # one decimal: ties
    labels = rng.integers(0, 5, rows).astype(np.float64)
    labels[last:] = 2.0                                        # a group of equal labels: no pair
    tp, tm = rng.uniform(0.25, 4.0, P), rng.uniform(0.25, 4.0, P)
    cfg = {"truncation": 3, "sigma": 1.5, "position_bias": {"positions": P}}
    want = TB.gradients(scores, labels, off, tp, tm, sigma=1.5, truncation=3)
    got = lambdarank_gradients(scores, labels, off, ctx=ctx, t_plus=tp, t_minus=tm, **cfg)
    for name, a, b in zip(("g", "h", "cost_plus", "cost_minus"), got, want):
        same_bits(a, b, name)
    assert not got[2][last:].any() and not got[3][last:].any()
    if n > 3:
        assert got[2].any() and got[3].any()


def fit_data(zero_first):
    X, y, off = T.dataset(5, rows=400, lo=5, hi=70)
    if zero_first:                                             # the item shown first is never the clicked side of a pair
        y[off[:-1]] = 0.0
    return X, y, off


@pytest.mark.parametrize("zero_first", [False, True])
@pytest.mark.parametrize("backend", ["lightgbm", "xgboost"])
def test_biased_fit_against_the_restatement(ctx, backend, zero_first):
    X, y, off = fit_data(zero_first)
    cfg = {"iterations": 6, "maxDepth": 3, "position_bias": {"positions": 8}}
    cfg.update({"backend": "xgboost", "min_child_weight": 1e-3} if backend == "xgboost" else {"numLeaves": 8, "min_data_in_leaf": 5})
    want = TB.fit(X, y, off, cfg=cfg)
    assert want["iterations_run"] == 6 and not np.array_equal(want["t_minus"], np.ones(8))
    if zero_first:
        assert all(Qp[0] == 0 and Qp.any() for Qp, _ in want["sums"]) and np.array_equal(want["t_plus"], np.ones(8))
    else:
        assert not np.array_equal(want["t_plus"], np.ones(8))
    _, hist = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    assert hist["model"] == want["model"]
    same_bits(hist["scores"], want["scores"], "scores")
    same_bits(hist["position_bias"][0], want["t_plus"], "t_plus")
    same_bits(hist["position_bias"][1], want["t_minus"], "t_minus")


@pytest.mark.parametrize("backend", ["lightgbm", "xgboost"])
def test_a_null_position_bias_is_no_position_bias(ctx, backend):
    X, y, off = fit_data(False)
    cfg = {"iterations": 3, "backend": backend}
    _, plain = fit_lambdamart(X, y, off, ctx=ctx, **cfg)
    _, null = fit_lambdamart(X, y, off, ctx=ctx, position_bias=None, **cfg)
    assert null["model"] == plain["model"] and len(null["position_bias"][0]) == 0
    same_bits(null["scores"], plain["scores"], "scores")
