"""Micro-benchmark of the LambdaMART fit on the device (mrk_train_*, csrc/train.hip): 100 000 groups of 10 ... 100 rows x 24 columns
(workloads/synth.py synthetic_ranking_rows: standard normal cells, 5 % NaN in four columns, labels 0 ... 4 that follow three columns
plus noise), 100 iterations of 16 leaves.
Deterministic seed.

Reported: the host clock around mrk_train_set (bins on the host, upload in pieces, the binning kernel) and around mrk_train_fit, and
inside them the HIP-event phases of mrk_profile_get - train_bin, train_grad (LambdaRank, max, quantise), train_hist, train_scan
(scan + pick), train_apply (leaf_of and score updates), train_eval (with --valid) -; what the fit's host clock holds beyond its
device phases, per scan (the record read back after every split is a stream synchronisation: this is its price together with the
host's book-keeping); the restatement (tests/train_reference.py) for ONE iteration on the first --ref-groups groups of the same data on
this host; and, if sklearn is importable, HistGradientBoostingRegressor's time per tree on the same matrix (a regressor on the labels:
context only, another objective).  No threshold: nothing was measured before this tool existed.
--categorical N declares the last N columns categorical (their cells rounded to ids 0 ... 49): the split search of those columns is
include/mrk.h's step 5c, the restatement and sklearn then see the rounded columns as numbers.
--backend xgboost [--depth D] fits the same matrix with the level-wise grower (include/mrk.h steps 2x, 5x, 6x, 7x; --leaves is unused):
the phases are then train_level_hist, train_level_scan (scan + pick), train_level_split (the per-tree start and one routing pass per
level), train_level_readback (the level's records copied back: one stream synchronisation each) and train_apply; `launches` holds the
launch count of every phase and the bounds they must keep - for T trees of depth D at most T x D histogram launches, scan launches and
read-backs - and the tool exits 1 when a count is above its bound.  The restatement is then tests/train_xgb_reference.py.
--device-set measures the hand-over alone, on the same matrix, alternating three times in one call: (a) mrk_train_set from the host
(bins on the host, upload in pieces) and (b) the matrix already in device memory - placed there outside the clock, as a values batch
leaves it -, appended in 16 pieces and sealed (include/mrk.h step 2d: bins on the device).  Per run: the host clock around the
hand-over, the HIP-event phases of step 2d's kernels (train_stage, train_check, train_keys, train_sort, train_cuts,
train_cat_counts, train_bin), the clock around the fit and the SHA-256 of the fitted model; the tool exits 1 unless every model is
the same.
  python tools/train_bench.py [--json] [--device-set] [--backend lightgbm|xgboost] [--depth D] [--groups N] [--min-items N] [--max-items N] [--iterations N] [--leaves N] [--ref-groups N] [--valid]
                              [--categorical N] [--device-set]
"""
import argparse
import hashlib
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
from metarank_amd.train import Trainer  # noqa: E402
import train_reference as T  # noqa: E402
import train_xgb_reference as TX  # noqa: E402
from workloads import synth  # noqa: E402

TIMERS = ("train_bin", "train_grad", "train_hist", "train_scan", "train_apply", "train_eval")
LEVEL_TIMERS = ("train_bin", "train_grad", "train_level_hist", "train_level_scan", "train_level_split", "train_level_readback", "train_apply", "train_eval")
COLS = 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--groups", type=int, default=100_000)
    ap.add_argument("--min-items", type=int, default=10)
    ap.add_argument("--max-items", type=int, default=100)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--leaves", type=int, default=16)
    ap.add_argument("--ref-groups", type=int, default=2000, help="groups of the restatement's one iteration (0: skip it)")
    ap.add_argument("--valid", action="store_true", help="a validation set of a tenth of the groups (early stopping stays out of reach)")
    ap.add_argument("--categorical", type=int, default=0, help="declare the last N columns categorical; their cells are rounded to ids 0 ... 49 (NaN stays)")
    ap.add_argument("--backend", choices=("lightgbm", "xgboost"), default="lightgbm")
    ap.add_argument("--depth", type=int, default=8, help="maxDepth of the xgboost backend")
    ap.add_argument("--device-set", action="store_true", help="mrk_train_set from the host against append + seal from device memory, three runs each")
    a = ap.parse_args()
    xgb = a.backend == "xgboost"
    timers = LEVEL_TIMERS if xgb else TIMERS
    ctx = M.Context(0)
    X, y, off = synth.synthetic_ranking_rows(a.groups, a.min_items, a.max_items, COLS, seed=0)
    rows = int(off[-1])
    cfg = {"iterations": a.iterations, "numLeaves": a.leaves, "early_stopping": a.iterations}
    if xgb:
        cfg = {"backend": "xgboost", "iterations": a.iterations, "maxDepth": a.depth, "early_stopping": a.iterations}
    cats = list(range(COLS - a.categorical, COLS))
    if cats:                                                              # (without the option the config has no `categorical` key)
        X[:, cats] = np.clip(np.rint((X[:, cats] + 3.0) * (49.0 / 6.0)), 0.0, 49.0)
        cfg["categorical"] = cats
    out = {"groups": a.groups, "rows": rows, "items_per_group": [a.min_items, a.max_items], "columns": COLS, "iterations": a.iterations, "leaves": a.leaves,
           "backend": a.backend, "depth": a.depth if xgb else None, "categorical": cats, "build": N.lib().mrk_build_id().decode()}
    if a.device_set:
        return device_set(a, ctx, cfg, out, X, y, off)

    ctx.profile_enable(True)
    t = Trainer(cfg, ctx)
    t0 = time.perf_counter()
    t.set(0, X, y, off)
    if a.valid:
        t.set(1, *synth.synthetic_ranking_rows(max(a.groups // 10, 1), a.min_items, a.max_items, COLS, seed=1))
    out["set_call_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    t.fit()
    out["fit_call_ms"] = (time.perf_counter() - t0) * 1e3
    parts = {name: ctx.profile_get(name) for name in timers}
    ctx.profile_enable(False)
    hist = t.history()
    model = t.model()
    t.close()
    for name in timers:
        out[name + "_ms"], out[name + "_launches"] = parts[name]
    out["trees"], out["best_iteration"] = hist["iterations_run"], hist["best_iteration"]
    out["model_sha256"] = hashlib.sha256(model).hexdigest()               # (two builds that fit the same forest print the same digest)
    if xgb:
        return finish_xgboost(a, ctx, out, parts, hist, model, X, y, off, rows)
    out["categorical_nodes"] = sum(int(b.split("num_cat=")[1].split("\n")[0]) for b in model.decode().split("Tree=")[1:])
    out["splits"] = sum(len(b.split("split_feature=")[1].split("\n")[0].split()) for b in model.decode().split("Tree=")[1:])
    scans = parts["train_scan"][1]                                        # (one timer spans a scan and its pick)
    device_ms = sum(parts[name][0] for name in TIMERS if name != "train_bin")
    out["fit_device_phases_ms"] = device_ms
    out["fit_host_and_sync_ms_per_scan"] = (out["fit_call_ms"] - device_ms) / max(scans, 1)
    out["fit_ms_per_tree"] = out["fit_call_ms"] / max(hist["iterations_run"], 1)

    if a.ref_groups > 0:
        g = min(a.ref_groups, a.groups)
        r = int(off[g])
        t0 = time.perf_counter()
        T.fit(X[:r], y[:r], off[:g + 1], cfg={"iterations": 1, "numLeaves": a.leaves})
        out["restatement_one_iteration_ms"] = (time.perf_counter() - t0) * 1e3
        out["restatement_rows"] = r
        out["restatement_us_per_row_iteration"] = out["restatement_one_iteration_ms"] * 1e3 / r
        out["device_us_per_row_iteration"] = out["fit_call_ms"] * 1e3 / (rows * max(hist["iterations_run"], 1))
    try:
        from sklearn.ensemble import HistGradientBoostingRegressor
    except ImportError:
        out["sklearn"] = None
    else:
        trees = 10
        t0 = time.perf_counter()
        HistGradientBoostingRegressor(max_iter=trees, max_leaf_nodes=a.leaves, early_stopping=False).fit(X, y)
        out["sklearn_hist_gbr_ms_per_tree"] = (time.perf_counter() - t0) * 1e3 / trees
    ctx.close()
    print(json.dumps(out) if a.json else json.dumps(out, indent=1))


SET_TIMERS = ("train_stage", "train_check", "train_keys", "train_sort", "train_cuts", "train_cat_counts", "train_bin")
DEVICE_PIECES = 16


def device_set(a, ctx, cfg, out, X, y, off):
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    X = np.ascontiguousarray(X, dtype=np.float64)
    rows, cols = X.shape
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), X.nbytes) == 0 and hip.hipMemcpy(d, X.ctypes.data, X.nbytes, 1) == 0   # outside the clock
    cuts = [rows * i // DEVICE_PIECES for i in range(DEVICE_PIECES + 1)]
    runs = {"host": [], "device": []}
    for _ in range(3):
        for path in ("host", "device"):
            ctx.profile_enable(True)                                      # (clears the phases)
            t = Trainer(cfg, ctx)
            t0 = time.perf_counter()
            if path == "host":
                t.set(0, X, y, off)
            else:
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    if hi > lo:
                        t.append_device(0, d.value + lo * cols * 8, hi - lo, cols)
                t.seal(0, y, off)
            run = {"set_call_ms": (time.perf_counter() - t0) * 1e3}
            for name in SET_TIMERS:
                run[name + "_ms"], run[name + "_launches"] = ctx.profile_get(name)
            t0 = time.perf_counter()
            t.fit()
            run["fit_call_ms"] = (time.perf_counter() - t0) * 1e3
            run["model_sha256"] = hashlib.sha256(t.model()).hexdigest()
            t.close()
            ctx.profile_enable(False)
            runs[path].append(run)
    hip.hipFree(d)
    out["device_pieces"] = DEVICE_PIECES
    out["runs"] = runs
    for path in runs:
        for key in ("set_call_ms", "fit_call_ms"):
            v = [r[key] for r in runs[path]]
            out[f"{path}_{key}"] = {"min": min(v), "median": sorted(v)[1], "max": max(v)}
    out["device_phases_ms"] = {name: sorted(r[name + "_ms"] for r in runs["device"])[1] for name in SET_TIMERS}
    hashes = {r["model_sha256"] for path in runs for r in runs[path]}
    out["model_sha256"] = {path: runs[path][0]["model_sha256"] for path in runs}
    out["models_equal"] = len(hashes) == 1
    out["set_speedup_median"] = out["host_set_call_ms"]["median"] / out["device_set_call_ms"]["median"]
    ctx.close()
    print(json.dumps(out) if a.json else json.dumps(out, indent=1))
    if not out["models_equal"]:
        sys.exit(1)


def finish_xgboost(a, ctx, out, parts, hist, model, X, y, off, rows):
    trees = json.loads(model)["learner"]["gradient_booster"]["model"]["trees"]
    out["nodes"] = sum(int(t["tree_param"]["num_nodes"]) for t in trees)
    out["splits"] = sum(sum(1 for l in t["left_children"] if l >= 0) for t in trees)
    bound = hist["iterations_run"] * a.depth                             # derived: one launch / read-back per level that can still split
    counts = {name: int(parts[name][1]) for name in LEVEL_TIMERS}
    out["launches"] = {"per_phase": counts, "bound_trees_x_depth": bound, "histogram": counts["train_level_hist"], "scan": counts["train_level_scan"],
                       "record_readbacks": counts["train_level_readback"]}
    out["launches"]["within_bound"] = all(out["launches"][k] <= bound for k in ("histogram", "scan", "record_readbacks"))
    device_ms = sum(parts[name][0] for name in LEVEL_TIMERS if name != "train_bin")
    out["fit_device_phases_ms"] = device_ms
    out["fit_host_and_sync_ms_per_readback"] = (out["fit_call_ms"] - device_ms) / max(counts["train_level_readback"], 1)
    out["fit_ms_per_tree"] = out["fit_call_ms"] / max(hist["iterations_run"], 1)
    if a.ref_groups > 0:
        g = min(a.ref_groups, a.groups)
        r = int(off[g])
        t0 = time.perf_counter()
        TX.fit(X[:r], y[:r], off[:g + 1], cfg={"iterations": 1, "maxDepth": a.depth})
        out["restatement_one_iteration_ms"] = (time.perf_counter() - t0) * 1e3
        out["restatement_rows"] = r
        out["restatement_us_per_row_iteration"] = out["restatement_one_iteration_ms"] * 1e3 / r
        out["device_us_per_row_iteration"] = out["fit_call_ms"] * 1e3 / (rows * max(hist["iterations_run"], 1))
    ctx.close()
    print(json.dumps(out) if a.json else json.dumps(out, indent=1))
    if not out["launches"]["within_bound"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
