"""The median of a numeric `diversity` over a whole large request, on the device (csrc/select.hip) against on the host
(MRK_DIVERSITY_SELECT=0: walk + std::sort of the mirror): ONE request of n candidates over the Ranklens model with one added
`diversity` feature of top = n.  Both settings in one process on one box, interleaved within every repetition; per setting the
host clock around mrk_rank (it ends in a device synchronise), around mrk_batch_load + run + fetch with flat ids (setting 0 falls
back to host lookups there), and the HIP-event timers "median" / "prepass".  The specialised kernels are off (MRK_RANK_JIT=0): the
added feature makes a new program, whose background compile would run beside the first repetitions.
  python tools/median_bench.py [n ...] [--reps 7] [--calls 20] [--once SETTING: one mrk_rank per size, for a kernel trace]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("MRK_RANK_JIT", "0")
import metarank_amd as M  # noqa: E402
from metarank_amd.ranker import HipRanker  # noqa: E402
from workloads import ranklens, synth  # noqa: E402

CATALOGUE, SESSIONS = 100_000, 10_000


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[100_000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--once", choices=["0", "1"], default=None)
    args = ap.parse_args()
    cfg = ranklens.ranklens_config()
    cfg["features"].append({"name": "divers_all", "type": "diversity", "source": "item.popularity", "top": max(args.sizes)})
    cfg["models"]["xgboost"]["features"].append("divers_all")
    ctx = M.Context(0)
    ranker = HipRanker(cfg, ctx)
    ranklens.load_state(ranker, ranklens.generate_state(CATALOGUE, SESSIONS))
    dim = ranker.dim("xgboost")
    booster = M.HipBooster(synth.synthetic_lgbm_model(n_trees=200, n_features=dim), M.LIGHTGBM, ctx)
    out = {}

    def setting(v):
        os.environ["MRK_DIVERSITY_SELECT"] = v
        M.reload_switches()

    for n in args.sizes:
        ev = ranklens.generate_requests(1, n, CATALOGUE, SESSIONS)[0]
        req, flat = M.Request(ev), M.RequestSet([ev])
        batch = ranker.new_batch()

        def rank_once():
            t = time.perf_counter()
            _, scores, _ = ranker.rerank("xgboost", req, booster)
            return (time.perf_counter() - t) * 1e3, scores

        def batch_once():
            t = time.perf_counter()
            batch.load("xgboost", flat)
            batch.run(booster)
            scores = batch.fetch()[0]
            return (time.perf_counter() - t) * 1e3, scores

        if args.once is not None:
            setting(args.once)
            rank_once()
            continue
        res = {v: {"rank_ms": [], "flat_batch_ms": [], "median_ms": [], "prepass_ms": []} for v in ("0", "1")}
        ref = None
        for rep in range(args.reps + 1):   # (repetition 0 warms every shape up and is dropped)
            for v in ("0", "1"):
                setting(v)
                ctx.profile_enable(True)
                t_rank, t_flat = [], []
                for _ in range(args.calls):
                    ms, scores = rank_once()
                    t_rank.append(ms)
                    ref = scores.copy() if ref is None else ref
                    assert np.array_equal(scores, ref), "the two settings disagree"
                calls_timed = args.calls
                med, k_med = ctx.profile_get("median")
                pre, k_pre = ctx.profile_get("prepass")
                for _ in range(args.calls):
                    ms, scores = batch_once()
                    t_flat.append(ms)
                    assert np.array_equal(scores, ref), "flat ids disagree"
                ctx.profile_enable(False)
                if rep == 0:
                    continue
                res[v]["rank_ms"].append(float(np.median(t_rank)))
                res[v]["flat_batch_ms"].append(float(np.median(t_flat)))
                res[v]["median_ms"].append(med / max(k_med, 1) if k_med else 0.0)
                res[v]["prepass_ms"].append(pre / max(k_pre, 1))
                assert k_med == (calls_timed if v == "1" else 0), (v, k_med)
        out[str(n)] = {v: {k: stats(x) for k, x in r.items()} for v, r in res.items()}
        print(n, json.dumps(out[str(n)]), flush=True)
        batch.close()
    os.environ.pop("MRK_DIVERSITY_SELECT", None)
    M.reload_switches()
    print(json.dumps({"median_bench": out, "reps": args.reps, "calls": args.calls}))


if __name__ == "__main__":
    main()
