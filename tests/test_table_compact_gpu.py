"""GPU: the compact 4-byte pre-pass table entries of the plain workgroup-per-request kernel (mrk_jit_rank_cells, csrc/table32_device.hpp)
and the rule that decides which batches get them (features.hpp compact_table_ok; capi_rank.cpp run_batch) - bit for bit against the
oracle and against the interpreting kernel (MRK_RANK_JIT=0: 8-byte entries), on the small state of test_table_bounds_gpu.py's
shape: vocabularies of 1 / 3 / ~40 tokens, sessions of 0 / 1 / 37 / 100 clicks, lists past MRK_IW_TOK = 5 and TOK_BATCH = 8, plus
one session whose 100 clicks insert exactly 2 047 tokens - all the same one - into one table.  Every case asks the debug export
which form ran and checks the launch's dynamic LDS bytes against the formula of launch_shape.hpp fused_lds_bytes.
One config: the specialised kernels compile once per module (MRK_RANK_JIT=1 waits for them)."""
import os

import numpy as np
import pytest

from backends import HipBackend, OracleBackend
import metarank_amd as M
from workloads import ranklens, synth

N_ITEMS = 300
N_BIG = 100                             # items 300 .. 399: the only ones with a `big` list, clicked by session "sbig" alone
FIELDS = ["g3", "v40", "one", "big"]
SWITCHES = ("MRK_RANK_FUSED", "MRK_RANK_JIT", "MRK_FUSED_SLICES", "MRK_FUSED_SPLIT", "MRK_FUSED_THREADS")
PLAIN, SPLIT, INTERPRETING = 1, 2, 0   # mrk_debug_batch_launch's kernel


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def lds_formula(i):
    """launch_shape.hpp fused_lds_bytes: tables (rounded up to 8 B) | median values | 32 PrepOut of 24 B | 96 ints | 16 | the larger of the
    threshold staging buffers and the resident threshold tables (when they fit the kernel's limit: 8 KB plain, 20 KB split)"""
    staging = (i["threads"] + 63) // 64 * 2 * i["thr_cap"] * 8
    rt = i["rt_bytes"] if i["rt_bytes"] <= (20480 if i["split"] else 8192) else 0
    return ((i["tab_entries"] * i["entry_bytes"] + 7) & ~7) + i["vals_cap"] * 8 + 32 * 24 + 96 * 4 + 16 + max(staging, rt)


def config():
    features = [
        {"name": "pop", "type": "number", "scope": "item", "source": "metadata.pop"},
        {"name": "prof", "type": "interacted_with", "interaction": "click", "field": [f"item.{f}" for f in FIELDS], "field_order": FIELDS,
         "scope": "session", "count": 100, "duration": "24h"},
        {"name": "div_g3", "type": "diversity", "source": "item.g3"},
        {"name": "div_v40", "type": "diversity", "source": "item.v40"},
        {"name": "div_one", "type": "diversity", "source": "item.one"},
        {"name": "div_price", "type": "diversity", "source": "item.price"},
    ]
    return {"features": features, "models": {"m": {"type": "lambdamart", "backend": {"type": "lightgbm", "iterations": 10}, "features": [f["name"] for f in features]}}}


def state(seed=12):
    rng = np.random.Generator(np.random.PCG64(seed))
    puts = []
    for i in range(N_ITEMS):
        if rng.random() < 0.08:
            continue   # an item without state
        puts.append(("double", f"item={i}/pop", float(rng.integers(0, 1000))))
        puts.append(("double", f"item={i}/div_price", float(rng.integers(0, 500)) / 4))
        puts.append(("string_list", f"item={i}/prof_g3", [f"g{t}" for t in rng.integers(0, 3, int(rng.integers(0, 4)))]))
        puts.append(("string_list", f"item={i}/prof_v40", [f"v{t}" for t in rng.integers(0, 40, int(rng.integers(0, 13)))]))   # up to 12: past IW_TOK and TOK_BATCH
        puts.append(("string_list", f"item={i}/prof_one", ["only"]))
        puts.append(("string_list", f"item={i}/div_g3", [f"g{t}" for t in rng.integers(0, 3, int(rng.integers(1, 4)))]))
        puts.append(("string_list", f"item={i}/div_v40", [f"v{t}" for t in rng.integers(0, 40, int(rng.integers(1, 13)))]))
        puts.append(("string", f"item={i}/div_one", "only"))
        if i % 3 == 0:   # candidates that hold the token the big session counted
            puts.append(("string_list", f"item={i}/prof_big", ["x"] * int(rng.integers(1, 11))))
    # 100 items x 20 tokens + 47 more = 2 047 insertions of ONE token: the last count the compact entry holds
    for k in range(N_BIG):
        puts.append(("double", f"item={N_ITEMS + k}/pop", float(k)))
        puts.append(("string_list", f"item={N_ITEMS + k}/prof_big", ["x"] * (21 if k < 47 else 20)))
    sessions = {s: [str(x) for x in rng.integers(0, N_ITEMS, ln)] for s, ln in (("s1", 1), ("s100", 100), ("s37", 37))}   # ("s0": nothing was put for it)
    sessions["sbig"] = [str(N_ITEMS + k) for k in range(N_BIG)]
    for s, v in sessions.items():
        puts.append(("bounded_list", f"session={s}/prof_interactions", v))
    return puts


ONE_MORE = ("string_list", f"item={N_ITEMS}/prof_big", ["x"] * 22)   # item 300: 21 -> 22 tokens, the session's table 2 047 -> 2 048 insertions


def request(name, session, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = rng.choice(N_ITEMS, size=n, replace=False)
    items = [{"id": (str(x) if rng.random() >= 0.03 else f"unknown{x}")} for x in ids]
    return {"id": name, "timestamp": ranklens.TS, "user": "u", "session": session, "fields": [], "items": items}


@pytest.fixture(scope="module")
def world():
    """the state, the oracle's answers for every distinct request (computed once, never changed), the forest"""
    cfg, puts = config(), state()
    orc = OracleBackend(cfg, "m")
    ranklens.load_state(orc, puts)
    distinct = {"a": request("a", "s100", 70, 1), "b": request("b", "s1", 70, 2), "c": request("c", "s0", 70, 3), "f": request("f", "s37", 70, 6),
                "d": request("d", "s100", 130, 4), "g": request("g", "sbig", 70, 7)}
    mats = {k: orc.matrix(ev) for k, ev in distinct.items()}
    allm = np.concatenate(list(mats.values()))
    blob = synth.synthetic_lgbm_model(n_trees=60, n_features=allm.shape[1], quantiles=ranklens.column_quantiles(allm), missing="per_feature")
    orc.load_model(blob, 0)
    expected = {k: orc.rerank(ev) for k, ev in distinct.items()}
    # the same state with one more insertion into the big session's table: the answers for that request, from an oracle of its own
    orc2 = OracleBackend(cfg, "m")
    ranklens.load_state(orc2, puts + [ONE_MORE])
    orc2.load_model(blob, 0)
    more = {"mat": orc2.matrix(distinct["g"]), "exp": orc2.rerank(distinct["g"])}
    orc2.close()
    return {"cfg": cfg, "puts": puts, "reqs": distinct, "mats": mats, "blob": blob, "expected": expected, "more": more}


def run_batch(hip, names, w, kernel, qualifies, what, override=None):
    """ranks the batch, checks results against the oracle bit for bit, the form that ran and the launch's LDS bytes"""
    reqs = [w["reqs"][n] for n in names]
    batch = hip.ranker.prepare("m", reqs)
    try:
        fused_entries, _ = batch.tables()
        batch.run(hip.booster)
        scores, order, _ = batch.fetch()
        info = batch.launch_info()
        print(what, info, "formula", lds_formula(info))
        assert (batch.status() == 0).all(), (what, batch.status())
        assert info["kernel"] == kernel and info["entry_bytes"] == (4 if kernel == PLAIN else 8) and info["qualifies"] == qualifies, (what, info)
        assert info["tab_entries"] == fused_entries and info["lds"] == lds_formula(info), (what, info, lds_formula(info))
        if kernel == PLAIN:   # half the tables' bytes of the same launch with wide entries (capacities are even)
            assert fused_entries % 2 == 0 and info["lds"] == lds_formula(dict(info, entry_bytes=8)) - fused_entries * 4, (what, info)
        for r, n in enumerate(names):
            _, es, eo = (override or {}).get(n, {}).get("exp") or w["expected"][n]
            lo, hi = batch.offsets[r], batch.offsets[r + 1]
            assert same(scores[lo:hi], es) and order[lo:hi].tolist() == eo.tolist(), (what, r, n)
        _, _, mat = batch.fetch(matrix=True)
        for r, n in enumerate(names):
            m = (override or {}).get(n, {}).get("mat")
            assert same(mat[batch.offsets[r]:batch.offsets[r + 1]], w["mats"][n] if m is None else m), (what, r, n)
        return scores, order
    finally:
        batch.close()


def set_switches(**kw):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(kw)
    M.reload_switches()


@pytest.fixture()
def switches():
    saved = {k: os.environ.get(k) for k in SWITCHES}
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    M.reload_switches()


def backend(w, extra=()):
    hip = HipBackend(w["cfg"], "m")
    ranklens.load_state(hip, w["puts"] + list(extra))
    hip.load_model(w["blob"], 0)
    assert hip.booster.info()["bitvector"] == 1
    return hip


@pytest.mark.gpu
def test_compact_and_wide_entries_give_the_oracles_bytes(world, switches):
    w = world
    hip = backend(w)
    try:
        full = ["a", "b", "c", "f"] * 17   # 68 requests of 70 candidates: past the op-split shapes, the plain kernel by the batch's own shape
        set_switches(MRK_RANK_JIT="1")
        s1, o1 = run_batch(hip, full, w, PLAIN, 1, "68x70 jit")
        run_batch(hip, ["a", "b", "c"], w, SPLIT, 1, "3x70 jit: op split")           # a handful of requests: the split kernel, wide
        set_switches(MRK_RANK_JIT="1", MRK_FUSED_SLICES="2", MRK_FUSED_SPLIT="1", MRK_FUSED_THREADS="64")
        run_batch(hip, ["d"], w, SPLIT, 1, "1x130 jit: two slices")
        set_switches(MRK_RANK_JIT="1", MRK_FUSED_SPLIT="1")                          # ... and the same handful made to take the plain kernel
        run_batch(hip, ["a", "b", "c"], w, PLAIN, 1, "3x70 jit: plain")
        set_switches(MRK_RANK_JIT="0")
        s0, o0 = run_batch(hip, full, w, INTERPRETING, 1, "68x70 interpreting")
        assert same(s1, s0) and o1.tolist() == o0.tolist()
    finally:
        hip.close()


@pytest.mark.gpu
def test_a_table_of_2047_insertions_is_compact_and_one_more_is_wide(world, switches):
    w = world
    hip = backend(w)
    try:
        set_switches(MRK_RANK_JIT="1", MRK_FUSED_SPLIT="1")
        assert M.debug_fused_lds(2047, 5)[0] and not M.debug_fused_lds(2048, 5)[0]
        run_batch(hip, ["g", "b"], w, PLAIN, 1, "2 047 insertions")
        assert np.nanmax(w["mats"]["g"]) >= 2047.0, "no candidate read the full counter"   # a candidate's `big` list of n tokens reads it n times
        ranklens.load_state(hip, [ONE_MORE])
        hip.ranker.flush()
        run_batch(hip, ["g", "b"], w, SPLIT, 0, "2 048 insertions", override={"g": w["more"]})
    finally:
        hip.close()


@pytest.mark.gpu
def test_a_column_that_saw_token_id_2_pow_20_is_wide(world, switches):
    w = world
    # four lists of 262 200 new tokens in a table's column, on items no request asks for: the store's token ids pass 2^20
    junk = [("string_list", f"item=junk{k}/div_one", [f"j{k}_{i}" for i in range(262_200)]) for k in range(4)]
    hip = backend(w, junk)
    try:
        set_switches(MRK_RANK_JIT="1", MRK_FUSED_SPLIT="1")
        assert hip.ranker.column_distinct("div_one") == 4 * 262_200 + 1
        run_batch(hip, ["a", "b", "c"], w, SPLIT, 0, "token id >= 2^20")
    finally:
        hip.close()
