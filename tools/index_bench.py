"""Micro-benchmark of the similar-items index (mrk_index_search, csrc/knn.hip): 1 M x 384 in both storage widths and
1 M x 100 in f64, at 1, 16 and 256 queries, n = 10.

Per case: the whole call (host clock around mrk_index_search, which ends in a device synchronise: upload of the queries,
norms, scan, selection, download), the scan kernel alone (HIP events, mrk_profile_get "knn_scan") and the selection
("knn_select"); the bytes the scan has to move = table bytes x query tiles of the launch (every tile of up to 8 queries
streams the table once) over the scan's time, against the 8 TB/s HBM figure of this repository's roofline; and the same
search by numpy on the host (BLAS products + argpartition - not bit-exact, the only baseline there is).
  python tools/index_bench.py [--json] [--rows N] [--quick] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metarank_amd as M  # noqa: E402
from metarank_amd.index import HipIndex  # noqa: E402

HBM_BPS = 8.0e12


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(np.min(ts))


def host_search(table, norms, queries, n):
    """cosine distance by BLAS, the n smallest by argpartition + sort"""
    qn = np.sqrt((queries * queries).sum(axis=1))
    d = 1.0 - (queries @ table.T) / (qn[:, None] * norms[None, :])
    part = np.argpartition(d, n, axis=1)[:, :n]
    return np.take_along_axis(part, np.argsort(np.take_along_axis(d, part, axis=1), axis=1), axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--quick", action="store_true", help="the f32 1 M x 384 case only, few repeats (profiler runs)")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy baseline")
    a = ap.parse_args()
    ctx = M.Context(0)
    rng = np.random.default_rng(0)
    rows, n = a.rows, 10
    out = {"rows": rows, "n": n, "cases": []}
    cases = [("f32", 384)] if a.quick else [("f32", 384), ("f64", 384), ("f64", 100)]
    for width, cols in cases:
        table = rng.standard_normal((rows, cols), dtype=np.float32)
        if width == "f64":
            table = table.astype(np.float64)
            table[0, 0] = 0.1          # one value that does not survive float: the table is stored as doubles
        t0 = time.perf_counter()
        ix = HipIndex.build([str(i) for i in range(rows)], table, ctx)
        build_s = time.perf_counter() - t0
        info = ix.info()
        assert info["stored_elem_bytes"] == (4 if width == "f32" else 8)
        norms = None
        for nq in (1, 16, 256):
            queries = rng.standard_normal((nq, cols))
            reps = 5 if (a.quick or nq == 256) else 20
            med, best = timed(lambda: ix.search(queries, n), reps)
            ctx.profile_enable(True)
            for _ in range(reps):
                ix.search(queries, n)
            scan_ms, scan_launches = ctx.profile_get("knn_scan")
            sel_ms, _ = ctx.profile_get("knn_select")
            ctx.profile_enable(False)
            tiles = (nq + 7) // 8 if nq > 4 else 1
            scan_s = scan_ms / 1e3 / reps
            moved = info["device_bytes"] * tiles
            case = {"storage": width, "cols": cols, "queries": nq, "table_bytes": info["device_bytes"], "build_s": build_s,
                    "call_ms_median": med * 1e3, "call_ms_min": best * 1e3, "scan_ms": scan_s * 1e3, "select_ms": sel_ms / reps,
                    "scan_launches_per_call": scan_launches / reps, "query_tiles": tiles, "scan_bytes_per_s": moved / scan_s,
                    "share_of_8TBps": moved / scan_s / HBM_BPS, "queries_per_s": nq / med}
            if not a.no_host and not a.quick:
                if norms is None:
                    norms = np.sqrt((table.astype(np.float64) ** 2).sum(axis=1)).astype(table.dtype)
                hq = queries.astype(table.dtype)     # a float32 table is searched in float32 on the host: its fastest form
                hmed, _ = timed(lambda: host_search(table, norms, hq, n), 2 if nq == 256 else 3, warm=1)
                got = ix.search(queries, n)[0]
                agree = float(np.mean([len(set(got[q].tolist()) & set(r.tolist())) / n for q, r in enumerate(host_search(table, norms, hq, n))]))
                case.update({"numpy_ms": hmed * 1e3, "speedup_vs_numpy": hmed / med, "top_n_overlap_with_numpy": agree})
            out["cases"].append(case)
            if not a.json:
                print(json.dumps(case), flush=True)
        ix.close()
        del table
    ctx.close()
    if a.json:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
