#!/usr/bin/env python
"""What a device-matched field_match column costs: the c2 workload (stock Ranklens model, 3 840 requests x 100 candidates)
against the same model with one `term` and one `bm25` column appended ("match": "device"), same process, runs
interleaved.  `python tools/match_bench.py [--requests N] [--items N] [--runs N] [--tokens N] [--query N]` prints one JSON
line: per-run wall times of mrk_batch_run + sync and the HIP-event time of the assembly kernel(s) for both models.
The defaults are a title-sized column; `--tokens 100 --query 128` is the worst the limits allow (lists of up to 200 tokens,
each looked up among 128 ids - 64 for the bm25 column)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import metarank_amd as M  # noqa: E402
from metarank_amd.ranker import HipRanker  # noqa: E402
from workloads import ranklens, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--requests", type=int, default=3840)
ap.add_argument("--items", type=int, default=100)
ap.add_argument("--catalogue", type=int, default=100_000)
ap.add_argument("--sessions", type=int, default=10_000)
ap.add_argument("--runs", type=int, default=8)
ap.add_argument("--tokens", type=int, default=6, help="stored tokens per item and column (1 .. 2 x this)")
ap.add_argument("--query", type=int, default=4, help="query tokens per request")
args = ap.parse_args()

vocab = sorted(f"t{i:05d}" for i in range(5000))
rng = np.random.Generator(np.random.PCG64(1))
dic = {"language": "en", "fields": ["title"], "docs": args.catalogue, "avgdl": float(args.tokens),
       "termfreq": {t: int(rng.integers(1, args.catalogue)) for t in vocab[::2]}}


def make(with_match):
    cfg = ranklens.ranklens_config()
    if with_match:
        for name, method in (("title_term", {"type": "term", "language": "en"}), ("title_bm25", {"type": "bm25", "language": "en", "termFreq": "tf"})):
            cfg["features"].append({"name": name, "type": "field_match", "match": "device", "rankingField": "ranking.query", "itemField": "item.title", "method": method})
            cfg["models"]["xgboost"]["features"].append(name)
    ctx = M.Context(0)
    r = HipRanker(cfg, ctx)
    ranklens.load_state(r, ranklens.generate_state(args.catalogue, args.sessions))
    if with_match:
        g = np.random.Generator(np.random.PCG64(2))
        for i in range(args.catalogue):
            toks = sorted(vocab[j] for j in g.choice(len(vocab), size=int(g.integers(1, 2 * args.tokens + 1)), replace=False))
            r.put_string_list(f"item={i}/title_term_title", toks)
            r.put_string_list(f"item={i}/title_bm25_title", toks)
        r.bind_termfreq("title_bm25", dic)
    r.flush()
    return ctx, r


reqs = ranklens.generate_requests(args.requests, args.items, args.catalogue, args.sessions)
g = np.random.Generator(np.random.PCG64(3))
sides = {}
for name in ("c2", "c2+match"):
    ctx, r = make(name != "c2")
    evs = reqs
    if name != "c2":
        evs = []
        for ev in reqs:
            q = sorted(vocab[j] for j in g.choice(len(vocab), size=args.query, replace=False))
            evs.append(dict(ev, fields=[{"name": "__tokens:title_term", "value": q}, {"name": "__tokens:title_bm25", "value": q[:64]}]))   # bm25's limit
    dim = r.dim("xgboost")
    booster = r.load_model(synth.synthetic_lgbm_model(n_trees=500, n_features=dim), 0)
    batch = r.prepare("xgboost", evs)
    for _ in range(3):
        batch.run(booster)
        batch.sync()
    sides[name] = {"ctx": ctx, "ranker": r, "batch": batch, "booster": booster, "wall_ms": []}
for _ in range(args.runs):   # interleaved: both models see the same clocks and neighbours
    for s in sides.values():
        t0 = time.perf_counter()
        s["batch"].run(s["booster"])
        s["batch"].sync()
        s["wall_ms"].append((time.perf_counter() - t0) * 1e3)
out = {"requests": args.requests, "items": args.items, "runs": args.runs, "tokens": args.tokens, "query": args.query, "build": M.lib().mrk_build_id().decode()}
for name, s in sides.items():
    s["ctx"].profile_enable(True)
    for _ in range(5):
        s["batch"].run(s["booster"])
        s["batch"].sync()
    kernels = {}
    for k in ("prepass", "assemble", "rank_fused", "score", "sort"):
        ms, n = s["ctx"].profile_get(k)
        if n:
            kernels[k] = round(ms / n, 4)
    s["ctx"].profile_enable(False)
    out[name] = {"wall_ms": [round(x, 4) for x in s["wall_ms"]], "median_wall_ms": round(float(np.median(s["wall_ms"])), 4), "kernel_avg_ms": kernels}
print(json.dumps(out), flush=True)
