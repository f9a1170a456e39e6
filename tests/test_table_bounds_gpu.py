"""GPU: pre-pass hash tables sized by the column's vocabulary (features.cpp table_capacity over min(insertions, twice the distinct
tokens of the column)) - against the oracle, bit for bit, on a small state whose columns have vocabularies of 1, 3 and ~40 tokens,
sessions of 0, 1 and 100 interactions and lists longer than the batches the kernels prefetch (MRK_IW_TOK = 5, TOK_BATCH = 8).
A 100-click session inserts hundreds of tokens into a table that can never hold more than 3 keys: the table has the
capacity of 6 (twice the bound: half the load factor, features.cpp), nothing overflows (status 0), and when later puts enlarge
the vocabulary a fresh batch's tables grow."""
import os

import numpy as np
import pytest

from backends import HipBackend, OracleBackend
import metarank_amd as M
from workloads import ranklens, synth

N_ITEMS = 300
FIELDS = ["g3", "v40", "one"]          # interacted_with fields: vocabulary 3, ~40, and one token everywhere
DIVS = ["div_g3", "div_v40", "div_one", "div_price"]
TOP = 20                                # DiversityFeature's default `top`
SWITCHES = ("MRK_RANK_FUSED", "MRK_RANK_JIT", "MRK_PREPASS_LDS", "MRK_FUSED_SLICES", "MRK_FUSED_SPLIT", "MRK_FUSED_THREADS")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def table_capacity(tokens: int, pct: int = 75) -> int:
    """features.cpp table_capacity"""
    inv = (100 * 65536 + pct - 1) // pct
    cap = ((tokens * inv) >> 16) + 2
    return max((cap + 1) & ~1, 8)


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


def state(seed=11):
    """(puts, item column -> {item: value}, session -> interacted items)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    puts, cols, sessions = [], {}, {}

    def put(kind, item, col, v):
        puts.append((kind, f"item={item}/{col}", v))
        cols.setdefault(col, {})[str(item)] = v

    for i in range(N_ITEMS):
        if rng.random() < 0.08:
            continue   # an item without state
        put("double", i, "pop", float(rng.integers(0, 1000)))
        put("double", i, "div_price", float(rng.integers(0, 500)) / 4)
        put("string_list", i, "prof_g3", [f"g{t}" for t in rng.integers(0, 3, int(rng.integers(0, 4)))])
        put("string_list", i, "prof_v40", [f"v{t}" for t in rng.integers(0, 40, int(rng.integers(0, 13)))])   # up to 12: past IW_TOK and TOK_BATCH
        put("string_list", i, "prof_one", ["only"])
        put("string_list", i, "div_g3", [f"g{t}" for t in rng.integers(0, 3, int(rng.integers(1, 4)))])
        put("string_list", i, "div_v40", [f"v{t}" for t in rng.integers(0, 40, int(rng.integers(1, 13)))])
        put("string", i, "div_one", "only")
    for s, ln in (("s1", 1), ("s100", 100), ("s37", 37)):   # ("s0": a session nothing was put for)
        sessions[s] = [str(x) for x in rng.integers(0, N_ITEMS, ln)]
        puts.append(("bounded_list", f"session={s}/prof_interactions", sessions[s]))
    return puts, cols, sessions


def request(name, session, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = rng.choice(N_ITEMS, size=n, replace=False)
    items = [{"id": (str(x) if rng.random() >= 0.03 else f"unknown{x}")} for x in ids]
    return {"id": name, "timestamp": ranklens.TS, "user": "u", "session": session, "fields": [], "items": items}


def expected_caps(ev, cols, sessions, distinct):
    """what features.cpp resolve_requests (host-resolved ids) sizes this request's tables to, in program order"""
    caps = []
    for f in FIELDS:
        col = cols.get("prof_" + f, {})
        count = sum(len(col.get(i, [])) for i in sessions.get(ev["session"], []))
        caps.append(table_capacity(min(count, 2 * distinct["prof_" + f])))
    for d in DIVS:
        col, tokens, taken = cols.get(d, {}), 0, 0
        for it in ev["items"]:
            if taken == TOP or d == "div_price":
                break
            v = col.get(it["id"])
            if v is not None:
                tokens += 1 if isinstance(v, str) else len(v)
                taken += 1
        caps.append(table_capacity(min(tokens, 2 * distinct.get(d, 0))))
    return caps


@pytest.fixture(scope="module")
def world():
    """the state, the oracle loaded with it, the requests and the oracle's answers - computed once, never changed"""
    cfg = config()
    puts, cols, sessions = state()
    orc = OracleBackend(cfg, "m")
    ranklens.load_state(orc, puts)
    batches = {"3x70": [request("a", "s100", 70, 1), request("b", "s1", 70, 2), request("c", "s0", 70, 3)],
               "1x130": [request("d", "s100", 130, 4)],
               "rank": [request("e", "s100", 100, 5), request("f", "s37", 70, 6)]}
    mats = {k: [orc.matrix(ev) for ev in v] for k, v in batches.items()}
    allm = np.concatenate([m for v in mats.values() for m in v])
    blob = synth.synthetic_lgbm_model(n_trees=60, n_features=allm.shape[1], quantiles=ranklens.column_quantiles(allm), missing="per_feature")
    orc.load_model(blob, 0)
    expected = {k: [orc.rerank(ev) for ev in v] for k, v in batches.items()}
    return {"cfg": cfg, "puts": puts, "cols": cols, "sessions": sessions, "orc": orc, "batches": batches, "mats": mats, "blob": blob, "expected": expected}


def true_distinct(cols):
    return {c: len({t for v in vals.values() for t in ([v] if isinstance(v, str) else v)}) for c, vals in cols.items() if c.startswith(("prof_", "div_")) and c != "div_price"}


def run_batch(hip, reqs, expected, mats, cols, sessions, distinct, what):
    batch = hip.ranker.prepare("m", reqs)
    try:
        fused_entries, caps = batch.tables()
        want = [expected_caps(ev, cols, sessions, distinct) for ev in reqs]
        print(what, "fused_entries", fused_entries, "caps", caps.tolist())
        assert caps.tolist() == want, what
        assert fused_entries == max(sum(w) for w in want), what
        batch.run(hip.booster)
        scores, order, _ = batch.fetch()
        assert (batch.status() == 0).all(), (what, batch.status())
        for r, (_, es, eo) in enumerate(expected):
            lo, hi = batch.offsets[r], batch.offsets[r + 1]
            assert same(scores[lo:hi], es) and order[lo:hi].tolist() == eo.tolist(), (what, r)
        _, _, mat = batch.fetch(matrix=True)
        for r in range(len(reqs)):
            assert same(mat[batch.offsets[r]:batch.offsets[r + 1]], mats[r]), (what, r)
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("jit", ["1", "0"])
def test_vocabulary_bounded_tables_match_the_oracle(world, jit):
    w = world
    hip = HipBackend(w["cfg"], "m")
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        ranklens.load_state(hip, w["puts"])
        hip.load_model(w["blob"], 0)
        assert hip.booster.info()["bitvector"] == 1
        # the tracker (first part: the CPU test pins it on the host alone): at least - here exactly - the column's vocabulary
        distinct = {c: hip.ranker.column_distinct(c) for c in true_distinct(w["cols"])}
        assert distinct == true_distinct(w["cols"])
        assert distinct["prof_g3"] == 3 and distinct["prof_one"] == 1 and distinct["div_one"] == 1 and 30 <= distinct["prof_v40"] <= 40
        # a 100-click session: hundreds of insertions, a table for 2 x 3 keys - and no smaller than one that holds the 3
        assert expected_caps(w["batches"]["3x70"][0], w["cols"], w["sessions"], distinct)[0] == table_capacity(6) == 10 >= table_capacity(3)
        # fused = one workgroup per request with LDS tables (two wavefronts, the second partial); "0" = the pre-pass kernel + the
        # item-parallel kernel, tables built in LDS and copied to the arena, or built in the arena (MRK_PREPASS_LDS=0)
        for fused, prepass_lds in (("1", "1"), ("0", "1"), ("0", "0")):
            os.environ.update(MRK_RANK_FUSED=fused, MRK_RANK_JIT=jit, MRK_PREPASS_LDS=prepass_lds)
            for k in ("MRK_FUSED_SLICES", "MRK_FUSED_SPLIT", "MRK_FUSED_THREADS"):
                os.environ.pop(k, None)
            M.reload_switches()
            run_batch(hip, w["batches"]["3x70"], w["expected"]["3x70"], w["mats"]["3x70"], w["cols"], w["sessions"], distinct, ("3x70", jit, fused, prepass_lds))
            if fused == "1":   # the sliced form: several one-wavefront workgroups per request, each building the request's tables
                os.environ.update(MRK_FUSED_SLICES="2", MRK_FUSED_SPLIT="1", MRK_FUSED_THREADS="64")
                M.reload_switches()
            run_batch(hip, w["batches"]["1x130"], w["expected"]["1x130"], w["mats"]["1x130"], w["cols"], w["sessions"], distinct, ("1x130", jit, fused, prepass_lds))
        for k in ("MRK_FUSED_SLICES", "MRK_FUSED_SPLIT", "MRK_FUSED_THREADS"):
            os.environ.pop(k, None)
        os.environ.update(MRK_RANK_FUSED="1", MRK_PREPASS_LDS="1")
        M.reload_switches()
        # mrk_rank: the one-launch kernel
        for ev, (_, es, eo) in zip(w["batches"]["rank"], w["expected"]["rank"]):
            _, scores, order = hip.ranker.rerank("m", ev, hip.booster)
            assert same(scores, es) and order.tolist() == eo.tolist(), ("mrk_rank", jit, ev["id"])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        M.reload_switches()
        hip.close()


@pytest.mark.gpu
def test_tables_grow_with_the_vocabulary(world):
    """more puts enlarge the vocabulary of the 3-token columns: after a flush a fresh batch's tables have grown and the
    results are still the oracle's (which gets the same puts in a copy of its own: the shared one stays as it is)"""
    w = world
    orc, hip = OracleBackend(w["cfg"], "m"), HipBackend(w["cfg"], "m")
    try:
        cols = {c: dict(v) for c, v in w["cols"].items()}
        more = []
        for i in range(0, N_ITEMS, 7):
            for c in ("prof_g3", "div_g3"):
                v = [f"new{(i // 7 + k) % 9}" for k in range(3)]
                more.append(("string_list", f"item={i}/{c}", v))
                cols[c][str(i)] = v
        reqs = w["batches"]["3x70"]
        for be in (orc, hip):
            ranklens.load_state(be, w["puts"])
            be.load_model(w["blob"], 0)
        before = {c: hip.ranker.column_distinct(c) for c in true_distinct(cols)}
        b0 = hip.ranker.prepare("m", reqs)
        _, caps0 = b0.tables()
        b0.close()
        for be in (orc, hip):
            ranklens.load_state(be, more)
        hip.ranker.flush()
        distinct = {c: hip.ranker.column_distinct(c) for c in true_distinct(cols)}
        assert distinct["prof_g3"] == before["prof_g3"] + 9 == 12 and distinct["prof_g3"] >= true_distinct(cols)["prof_g3"]
        expected = [orc.rerank(ev) for ev in reqs]
        run_batch(hip, reqs, expected, [e[0] for e in expected], cols, w["sessions"], distinct, "grown")
        b1 = hip.ranker.prepare("m", reqs)
        _, caps1 = b1.tables()
        b1.close()
        assert (caps1 >= caps0).all() and caps1[0, 0] == table_capacity(24) > caps0[0, 0] == table_capacity(6)
    finally:
        hip.close()
