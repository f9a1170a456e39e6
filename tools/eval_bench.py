"""Micro-benchmark of the evaluation that ends a train (mrk_model_eval, csrc/eval.hip): 100 000 groups of 10 ... 100 items x 24
columns scored with the benchmark forest (500 LightGBM trees of 16 leaves, as tools/score_bench.py builds it) and reduced to
ndcg@10 for the predicted scores, noopArray and random scores; then one group of 100 000 items.  Deterministic seed.

Reported per call: the host clock around mrk_model_eval (argument checks, gains and lg table, uploads in pieces, scoring, the three
evaluations, the mean) and inside it the HIP-event phases of mrk_profile_get - "eval_score" (the forest over every piece),
"eval_wave" (groups of up to 64 items, one wavefront each), "eval_group" (up to 4 096, one workgroup each), "eval_big" (beyond) -,
each over the three score arrays of a call; and the time tests/eval_reference.evaluate_numpy takes on this host for ONE of the
three evaluations (the predicted scores), with the largest difference between its values and the device's (numpy's sums are
pairwise: it is a clock, not an oracle).  No threshold: nothing was measured before this tool existed.
  python tools/eval_bench.py [--json] [--groups N] [--min-items N] [--max-items N] [--big N] [--trees N] [--reps N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import metarank_amd as M  # noqa: E402
from metarank_amd import _native as N  # noqa: E402
from metarank_amd.eval import eval_scores, evaluate  # noqa: E402
from workloads import synth  # noqa: E402
import eval_reference as E  # noqa: E402

TIMERS = ("eval_score", "eval_wave", "eval_group", "eval_big")
COLS = 24


def run(ctx, booster, X, labels, off, reps):
    """reps + 1 calls (the first warms up and is not counted): median wall ms, timers per call, the last call's result and scores"""
    walls, res, scores = [], None, None
    for k in range(reps + 1):
        if k == 1:
            ctx.profile_enable(True)
        t = time.perf_counter()
        res, scores = evaluate(booster, X, labels, off, [("ndcg", 10)], seed=1, return_scores=True)
        if k:
            walls.append(time.perf_counter() - t)
    parts = {name: ctx.profile_get(name) for name in TIMERS}
    ctx.profile_enable(False)
    return float(np.median(walls)) * 1e3, {k: (v[0] / reps, v[1] // reps) for k, v in parts.items()}, res[0], scores


def report(out, prefix, wall, parts, res, rows):
    out[prefix + "_rows"] = rows
    out[prefix + "_call_ms"] = wall
    for name in TIMERS:
        out[f"{prefix}_{name}_ms"] = parts[name][0]
        out[f"{prefix}_{name}_launches"] = parts[name][1]
    out[prefix + "_ndcg10"] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--groups", type=int, default=100_000)
    ap.add_argument("--min-items", type=int, default=10)
    ap.add_argument("--max-items", type=int, default=100)
    ap.add_argument("--big", type=int, default=100_000, help="items of the single large group (0: skip it)")
    ap.add_argument("--trees", type=int, default=500)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    ctx = M.Context(0)
    rng = np.random.default_rng(0)
    sample = rng.normal(size=(4096, COLS))
    q = [np.quantile(sample[:, j], np.linspace(0.02, 0.98, 49)) for j in range(COLS)]
    booster = M.HipBooster(synth.synthetic_lgbm_model(n_trees=a.trees, n_features=COLS, quantiles=q, missing="per_feature", cat_features=[7], cat_prob=0.007),
                           M.LIGHTGBM, ctx)
    out = {"groups": a.groups, "items_per_group": [a.min_items, a.max_items], "columns": COLS, "trees": a.trees, "build": N.lib().mrk_build_id().decode()}

    lens = rng.integers(a.min_items, a.max_items + 1, a.groups)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = int(off[-1])
    X = rng.normal(size=(rows, COLS))
    labels = rng.integers(0, 5, rows).astype(np.float64) * (rng.random(rows) < 0.1)
    wall, parts, res, scores = run(ctx, booster, X, labels, off, a.reps)
    report(out, "many", wall, parts, res, rows)
    out["many_groups_over_64_items"] = int((lens > 64).sum())
    t = time.perf_counter()
    host = E.evaluate_numpy(scores, labels, off, 10)
    out["many_numpy_one_evaluation_ms"] = (time.perf_counter() - t) * 1e3
    _, dev = eval_scores(scores, labels, off, "ndcg", 10, per_group=True, ctx=ctx)
    out["many_max_abs_diff_numpy"] = float(np.abs(dev - host).max())
    out["many_device_one_evaluation_ms"] = (parts["eval_wave"][0] + parts["eval_group"][0] + parts["eval_big"][0]) / 3.0
    del X

    if a.big > 0:
        off = np.array([0, a.big], dtype=np.int64)
        X = rng.normal(size=(a.big, COLS))
        labels = rng.integers(0, 5, a.big).astype(np.float64) * (rng.random(a.big) < 0.1)
        wall, parts, res, scores = run(ctx, booster, X, labels, off, a.reps)
        report(out, "big", wall, parts, res, a.big)
        t = time.perf_counter()
        host = E.evaluate_numpy(scores, labels, off, 10)
        out["big_numpy_one_evaluation_ms"] = (time.perf_counter() - t) * 1e3
        out["big_abs_diff_numpy"] = abs(res["value"] - float(host[0]))
    ctx.close()
    print(json.dumps(out) if a.json else json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
