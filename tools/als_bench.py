"""Micro-benchmark of the similar-items fit (mrk_als_*, csrc/als.hip): 1 M click-through pairs of 50 000 users over 10 000 items,
items Zipf s = 1.1, users Zipf s = 0.7, K = 100 factors (the reference's default), deterministic seed.

Reported: the add (host clock around mrk_als_add: interning of the ids), the fit (host clock around mrk_als_fit, which ends in a
device synchronise) and inside it the host's CSR / CSC build and initial factors (host clock, mrk_profile_get "als_host_problem" /
"als_host_init"), the two sweeps and the two K x K products (HIP events, "als_sweep_users" / "als_sweep_items" / "als_gram_items" /
"als_gram_users"; per launch = per iteration) and the pack into the index table with its norms ("als_pack"); the time per
iteration; and `--host-iterations` iterations of the vectorised numpy form of the restatement on this host
(tests/als_reference.fit_numpy), whose item-factor bits a device fit of that many iterations must equal.
  python tools/als_bench.py [--json] [--pairs N] [--users N] [--items N] [--factors K] [--iterations N] [--host-iterations N]
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
from metarank_amd.als import init_matrix  # noqa: E402
import als_reference as A  # noqa: E402

TIMERS = ("als_host_problem", "als_host_init", "als_gram_items", "als_sweep_users", "als_gram_users", "als_sweep_items", "als_pack")


def workload(n, users, items, seed):
    """(user index, item index) of n pairs, both numbered by first appearance: Zipf s = 0.7 over the users, s = 1.1 over the items"""
    rng = np.random.default_rng(seed)

    def draw(m, s):
        p = 1.0 / np.arange(1, m + 1) ** s
        v = rng.choice(m, size=n, p=p / p.sum())
        _, first = np.unique(v, return_index=True)
        seen = np.sort(first)
        rank = np.empty(m, dtype=np.int64)
        rank[v[seen]] = np.arange(len(seen))
        return rank[v], len(seen)

    u, nu = draw(users, 0.7)
    i, ni = draw(items, 1.1)
    return u, i, nu, ni


class Ids:
    """n pointers into one buffer of NUL-terminated ids"""

    def __init__(self, prefix, index, count):
        ids = [b"%s-%d" % (prefix, k) for k in range(count)]
        offs = np.concatenate([[0], np.cumsum([len(i) + 1 for i in ids])[:-1]]).astype(np.uint64)
        self.buf = C.create_string_buffer(b"\0".join(ids) + b"\0")
        self.ptrs = (np.uint64(C.addressof(self.buf)) + offs)[index]
        self.names = [i.decode() for i in ids]

    def arg(self):
        return C.cast(self.ptrs.ctypes.data, C.POINTER(C.c_char_p))


def device_fit(ctx, cfg, us, its, n, seed, reps):
    """add once, fit reps + 1 times (the first warms up and is not counted): (add ms, median fit ms, timers per fit, item factors)"""
    L = N.lib()
    b = C.c_void_p()
    N.check(L.mrk_als_begin(ctx.handle, json.dumps(cfg).encode(), C.byref(b)))
    t = time.perf_counter()
    N.check(L.mrk_als_add(b, us.arg(), its.arg(), n))
    add = time.perf_counter() - t
    fits, Q = [], None
    for k in range(reps + 1):
        if k == 1:
            ctx.profile_enable(True)
        h = C.c_void_p()
        t = time.perf_counter()
        N.check(L.mrk_als_fit(b, seed, None, None, None, C.byref(h)))
        if k:
            fits.append(time.perf_counter() - t)
        ix = M.HipIndex(h, ctx)
        if k == reps:
            Q = ix.vectors()
        ix.close()
    parts = {name: ctx.profile_get(name) for name in TIMERS}
    ctx.profile_enable(False)
    L.mrk_als_builder_free(b)
    return add * 1e3, (float(np.median(fits)) * 1e3 if fits else 0.0), {k: (v[0] / max(reps, 1), v[1] // max(reps, 1)) for k, v in parts.items()}, Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--users", type=int, default=50_000)
    ap.add_argument("--items", type=int, default=10_000)
    ap.add_argument("--factors", type=int, default=100)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--host-iterations", type=int, default=1, help="iterations of the numpy form (0: skip it)")
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    ctx = M.Context(0)
    out = {"pairs": a.pairs, "factors": a.factors, "iterations": a.iterations, "build": N.lib().mrk_build_id().decode()}
    u, i, nu, ni = workload(a.pairs, a.users, a.items, seed=0)
    us, its = Ids(b"user", u, nu), Ids(b"item", i, ni)
    cfg = {"factors": a.factors, "iterations": a.iterations}
    add, fit, parts, _ = device_fit(ctx, cfg, us, its, a.pairs, 1, a.reps)
    lens_u, lens_i = np.bincount(u), np.bincount(i)
    out.update({"users_seen": nu, "items_seen": ni, "distinct_pairs": int(len(np.unique(u * ni + i))), "longest_user_row_pairs": int(lens_u.max()),
                "longest_item_row_pairs": int(lens_i.max()), "add_ms": add, "fit_ms": fit})
    device = 0.0
    for name in TIMERS:
        ms, launches = parts[name]
        out[name + "_ms_per_fit"] = ms
        if name.startswith(("als_gram", "als_sweep")):
            out[name + "_ms_per_iteration"] = ms / max(launches, 1)
            device += ms / max(launches, 1)
    out["device_ms_per_iteration"] = device
    out["host_problem_share_of_fit"] = parts["als_host_problem"][0] / fit
    if a.host_iterations > 0:
        cfg_h = {"factors": a.factors, "iterations": a.host_iterations}
        _, _, _, Q = device_fit(ctx, cfg_h, us, its, a.pairs, 1, 0)
        users_l, items_l = [us.names[k] for k in u], [its.names[k] for k in i]
        pr = A.Problem(users_l, items_l)
        P0, Q0 = init_matrix(1, 0, nu, a.factors), init_matrix(1, 1, ni, a.factors)   # (the generator's bytes)
        t = time.perf_counter()
        _, Qn = A.fit_numpy(A.parse_config(cfg_h), pr, P0, Q0)
        out["numpy_ms_per_iteration"] = (time.perf_counter() - t) * 1e3 / a.host_iterations
        out["bits_equal_numpy"] = bool(np.array_equal(A.bits(Q), A.bits(Qn)))
        out["max_abs_diff_numpy"] = float(np.abs(Q - Qn).max())
        out["iteration_speedup_vs_numpy"] = out["numpy_ms_per_iteration"] / device
    ctx.close()
    print(json.dumps(out) if a.json else json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
