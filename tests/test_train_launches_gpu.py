"""GPU: the launch discipline of the LambdaMART fit (csrc/train_fit.cpp), which the byte comparisons of tests/test_train_gpu.py,
tests/test_train_cat_gpu.py and tests/test_train_xgb_gpu.py cannot see: a histogram built once too often, or a stream waited for once
too often, leaves the model as it is.  The context's profile counts the timed sections of a fit (mrk_profile_get); the counts they must
have are derived here from the returned model alone:
  lightgbm  a tree of L leaves takes one histogram and one scan for its root and one of each per split whose children can still be
            split - every split but the one that fills the tree: L - 1 of each when L == numLeaves, else L (maxDepth is out of reach
            here).  A fit that ends on a root that cannot split has paid that root's histogram and scan.
  xgboost   a tree whose deepest node has depth D takes one histogram, one scan and one read-back of records for every level that is
            scanned: levels 0 ... D, but never level maxDepth: min(D + 1, maxDepth) of each.
  both      one timed validation metric per tree grown, none without a validation set."""
import json

import pytest

import train_reference as T
import metarank_amd as M
from metarank_amd.train import fit_lambdamart

pytestmark = pytest.mark.gpu

ROWS, ITERATIONS = 1200, 5
PHASES = ("train_hist", "train_scan", "train_level_hist", "train_level_scan", "train_level_readback", "train_eval")


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def counted_fit(ctx, cfg, valid):
    """(history with the model, {phase: timed sections of this fit})"""
    X, y, off = T.dataset(1, rows=ROWS)
    ctx.profile_enable(True)                                               # (clears the counts of earlier fits)
    try:
        booster, hist = fit_lambdamart(X, y, off, valid=T.dataset(101, rows=300) if valid else None, ctx=ctx, **cfg)
        counts = {name: ctx.profile_get(name)[1] for name in PHASES}
    finally:
        ctx.profile_enable(False)
    if booster is not None:
        booster.close()
    # every iteration grows its tree here: the fit ends neither on an unsplittable root nor early, and without a validation set the
    # model holds every tree that was grown
    assert hist["iterations_run"] == ITERATIONS
    print(cfg, "valid" if valid else "", counts)
    return hist, counts


def check_eval(hist, counts, valid):
    assert counts["train_eval"] == (hist["iterations_run"] if valid else 0)


@pytest.mark.parametrize("categorical", [[], [3]], ids=["numeric", "categorical"])
def test_lightgbm_one_histogram_and_one_scan_per_splittable_split(ctx, categorical):
    cfg = {"numLeaves": 4, "maxDepth": 8, "iterations": ITERATIONS}
    if categorical:
        cfg["categorical"] = categorical
    hist, counts = counted_fit(ctx, cfg, valid=False)
    leaves = [int(block.split("num_leaves=")[1].split("\n")[0]) for block in hist["model"].decode().split("Tree=")[1:]]
    assert len(leaves) == ITERATIONS and all(2 <= n <= 4 for n in leaves)
    want = sum(n - 1 if n == 4 else n for n in leaves)
    assert counts["train_hist"] == want and counts["train_scan"] == want, (leaves, want)
    assert counts["train_level_hist"] == counts["train_level_scan"] == counts["train_level_readback"] == 0
    check_eval(hist, counts, False)
    vhist, vcounts = counted_fit(ctx, cfg, valid=True)
    assert vcounts["train_hist"] == vcounts["train_scan"] > 0
    check_eval(vhist, vcounts, True)


def depths(tree):
    """per node of one tree of XGBoost's JSON (a child's id is above its parent's)"""
    d = [0] * len(tree["parents"])
    for node in range(1, len(d)):
        d[node] = d[tree["parents"][node]] + 1
    return d


@pytest.mark.parametrize("max_depth", [3, 6])
def test_xgboost_one_histogram_scan_and_readback_per_scanned_level(ctx, max_depth):
    cfg = {"backend": "xgboost", "maxDepth": max_depth, "iterations": ITERATIONS}
    hist, counts = counted_fit(ctx, cfg, valid=False)
    trees = json.loads(hist["model"])["learner"]["gradient_booster"]["model"]["trees"]
    deepest = [max(depths(t)) for t in trees]
    assert len(deepest) == ITERATIONS and all(1 <= d <= max_depth for d in deepest)
    want = sum(min(d + 1, max_depth) for d in deepest)
    assert counts["train_level_hist"] == want and counts["train_level_scan"] == want and counts["train_level_readback"] == want, (deepest, want)
    assert counts["train_hist"] == counts["train_scan"] == 0
    check_eval(hist, counts, False)
    vhist, vcounts = counted_fit(ctx, cfg, valid=True)
    assert vcounts["train_level_hist"] == vcounts["train_level_scan"] == vcounts["train_level_readback"] > 0
    check_eval(vhist, vcounts, True)
