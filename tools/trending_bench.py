"""Micro-benchmark of the trending recommender's fit (mrk_trending_*, csrc/trending.hip): 10 M interactions over 100 000 items,
Zipf s = 1.1, 30 days, two weights, deterministic seed.

Reported: the upload (host clock around mrk_trending_add: interning of the ids on the host + the pinned pieces), the fit
(host clock around mrk_trending_fit, which ends in a device synchronise) and inside it the count, score and order launches (HIP
events, mrk_profile_get "trending_count" / "trending_score" / "trending_order"); interactions per second over upload + fit; and
the same fit by numpy on the host (tests/trending_reference.fit_numpy: np.add.at counts + the same ordered sum), whose order and
score bits the device's must equal.  `--ab`: the count kernel's two forms (wavefront-combined atomics, MRK_TRENDING_COUNT=plain:
one atomic per interaction) interleaved in this process on the workload and on a hot-item shape (half of all interactions on one
item today).
  python tools/trending_bench.py [--json] [--interactions N] [--items N] [--no-host] [--ab]
"""
import argparse
import ctypes as C
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
import trending_reference as T  # noqa: E402

DAY = T.DAY_MS
NOW = 1_700_000_000_000
CONFIG = {"weights": [{"interaction": "purchase", "weight": 5.0, "decay": 0.5, "window": "30d"},
                      {"interaction": "click", "weight": 1.0, "decay": 0.9, "window": "30d"}]}
TYPES = ["click", "purchase", "view"]


def workload(n, items, seed, hot=False):
    """(item index numbered by first appearance, type index, ts): Zipf s = 1.1 over the items, 80 / 15 / 5 % click / purchase /
    view, ts uniform over 30 days; hot: every second interaction is a click on one item within the last hour"""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, items + 1) ** 1.1
    item = rng.choice(items, size=n, p=p / p.sum())
    tix = rng.choice(3, size=n, p=[0.8, 0.15, 0.05]).astype(np.int32)
    ts = NOW - rng.integers(0, 30 * DAY, n)
    if hot:
        item[::2] = 0
        tix[::2] = 0
        ts[::2] = NOW - rng.integers(0, 3_600_000, len(ts[::2]))
    ts[0] = NOW
    _, first = np.unique(item, return_index=True)
    rank = np.empty(items, dtype=np.int64)
    seen = np.sort(first)
    rank[item[seen]] = np.arange(len(seen))
    return rank[item].astype(np.int64), tix, ts.astype(np.int64), len(seen)


class Stream:
    """the arrays mrk_trending_add takes, built once: 10 M pointers into one buffer of NUL-terminated ids"""

    def __init__(self, item, tix, ts, n_items):
        ids = [b"item-%d" % k for k in range(n_items)]
        offs = np.concatenate([[0], np.cumsum([len(i) + 1 for i in ids])[:-1]]).astype(np.uint64)
        self.buf = C.create_string_buffer(b"\0".join(ids) + b"\0")
        self.ptrs = (np.uint64(C.addressof(self.buf)) + offs)[item]
        self.names = (C.c_char_p * len(TYPES))(*[t.encode() for t in TYPES])
        self.tix, self.ts, self.n = np.ascontiguousarray(tix, dtype=np.int32), np.ascontiguousarray(ts, dtype=np.int64), len(item)

    def add(self, handle):
        N.check(N.lib().mrk_trending_add(handle, C.cast(self.ptrs.ctypes.data, C.POINTER(C.c_char_p)), self.names, len(TYPES),
                                         self.tix.ctypes.data, self.ts.ctypes.data, self.n))


def run(ctx, s, reps):
    """upload once, fit `reps` times (the builder stays valid): medians in ms"""
    L = N.lib()
    b = C.c_void_p()
    N.check(L.mrk_trending_begin(ctx.handle, json.dumps(CONFIG).encode(), C.byref(b)))
    t = time.perf_counter()
    s.add(b)
    upload = time.perf_counter() - t
    fits, model = [], None
    for k in range(reps + 1):                      # the first fit warms up (code objects, allocations) and is not counted
        if k == 1:
            ctx.profile_enable(True)
        h = C.c_void_p()
        t = time.perf_counter()
        N.check(L.mrk_trending_fit(b, C.byref(h)))
        if k:
            fits.append(time.perf_counter() - t)
        if model:
            L.mrk_trending_free(model)
        model = h
    parts = {k: ctx.profile_get("trending_" + k)[0] / reps for k in ("count", "score", "order")}
    ctx.profile_enable(False)
    L.mrk_trending_builder_free(b)
    return upload * 1e3, float(np.median(fits)) * 1e3, parts, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--interactions", type=int, default=10_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy baseline")
    ap.add_argument("--ab", action="store_true", help="the count kernel's two forms on the workload and the hot-item shape")
    a = ap.parse_args()
    ctx = M.Context(0)
    L = N.lib()
    out = {"interactions": a.interactions, "items": a.items, "build": L.mrk_build_id().decode()}
    item, tix, ts, n_items = workload(a.interactions, a.items, seed=0)
    s = Stream(item, tix, ts, n_items)
    upload, fit, parts, model = run(ctx, s, a.reps)
    out.update({"items_seen": n_items, "upload_ms": upload, "fit_ms": fit, "count_ms": parts["count"], "score_ms": parts["score"],
                "order_ms": parts["order"], "interactions_per_s": a.interactions / ((upload + fit) / 1e3),
                "interactions_per_s_fit_only": a.interactions / (fit / 1e3)})
    if not a.no_host:
        t = time.perf_counter()
        order, score = T.fit_numpy(CONFIG, item, tix, TYPES, ts, n_items)
        out["numpy_ms"] = (time.perf_counter() - t) * 1e3
        n = C.c_int32(0)
        got = np.zeros(n_items)
        N.check(L.mrk_trending_predict(model, n_items, got.ctypes.data, C.byref(n)))
        ids = [L.mrk_trending_id(model, k) for k in range(0, n_items, max(n_items // 1000, 1))]
        out["bits_equal_numpy"] = bool(n.value == n_items and np.array_equal(T.bits(got), T.bits(score[order])) and
                                       ids == [b"item-%d" % order[k] for k in range(0, n_items, max(n_items // 1000, 1))])
        out["fit_speedup_vs_numpy"] = out["numpy_ms"] / fit
    L.mrk_trending_free(model)
    if a.ab:
        out["ab"] = []
        for shape, hot in (("zipf", False), ("hot_item", True)):
            if hot:
                item, tix, ts, n_items = workload(a.interactions, a.items, seed=1, hot=True)
                s = Stream(item, tix, ts, n_items)
            row = {"shape": shape}
            for mode in ("combine", "plain", "combine", "plain"):           # interleaved, two rounds; the library reads the switch per fit
                os.environ["MRK_TRENDING_COUNT"] = mode
                _, _, parts, model = run(ctx, s, a.reps)
                L.mrk_trending_free(model)
                row.setdefault(mode + "_count_ms", []).append(parts["count"])
            os.environ.pop("MRK_TRENDING_COUNT")
            out["ab"].append(row)
    ctx.close()
    print(json.dumps(out) if a.json else json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
