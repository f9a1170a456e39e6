"""GPU: a request's pre-pass on all lanes of its workgroup (csrc/rank_device.hpp PRE_SIDE / PRE_SHARE: the string entries of a
diversity group side by side on wavefront 0, the interacted_with section as (item, field) tasks whose rounds the wavefronts claim from a
counter in LDS) - bit for bit against the oracle, against the interpreting kernel (MRK_RANK_JIT=0) and, for the main config, with the
two switches (MRK_JIT_DEFINES=MRK_PRE_SIDE=.. MRK_PRE_SHARE=..) at 0 and 1 against each other.  Batches of 3 requests over a small
catalogue: requests of 1 .. 130 candidates, sessions of 0 .. 100 interacted items and one that repeats a single item 100 times, 1 / 5 /
64 leading candidates without any diversity column (the continuation past the first 64), a numeric and a string-list entry in one
group, `top` 3 / 20 / 64 / 65 (65: the workgroup-wide path), five string entries (more than one pass) and a single one, three numeric
entries in one group (the segmented median), a list of 150 interacted items beside a second interacted_with list; the plain
kernel (compact tables), the op-split and the sliced kernel (wide tables) and a column that saw a token id >= 2^20 (wide).  Status 0
everywhere; the form that ran comes from mrk_debug_batch_launch."""
import os

import numpy as np
import pytest

from backends import HipBackend, OracleBackend
import metarank_amd as M
from workloads import ranklens, synth

N_ITEMS = 260
N_BARE = 64                              # items "bare0" .. "bare63": a record without any diversity column
FIELDS = ["g3", "v40", "one", "w9"]
SWITCHES = ("MRK_RANK_FUSED", "MRK_RANK_JIT", "MRK_FUSED_SLICES", "MRK_FUSED_SPLIT", "MRK_FUSED_THREADS", "MRK_JIT_DEFINES")
PLAIN, SPLIT, INTERPRETING = 1, 2, 0    # mrk_debug_batch_launch's kernel
SESSIONS = {"s1": 1, "s15": 15, "s16": 16, "s17": 17, "s64": 64, "s65": 65, "s100": 100}   # ("s0": nothing was put for it)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def config(kind):
    top = {"top3": 3, "top64": 64, "top65": 65}.get(kind)
    div = lambda col: dict({"name": f"div_{col}", "type": "diversity", "source": f"item.{col}"}, **({"top": top} if top else {}))
    cols = {"five": ["g3", "v40", "one", "w9", "z"], "single": ["v40"], "nums": ["price", "pop", "g3", "rank"], "lists": ["g3", "price"]}.get(kind, ["price", "g3", "v40", "one", "pop"])   # main: a number first, then a string list, in one group; `pop` is a second group
    features = [
        {"name": "pop", "type": "number", "scope": "item", "source": "metadata.pop"},
        {"name": "prof", "type": "interacted_with", "interaction": "click", "field": [f"item.{f}" for f in FIELDS], "field_order": FIELDS,
         "scope": "session", "count": 100, "duration": "24h"},
    ] + [div(c) for c in cols]
    if kind == "lists":   # a list longer than the 128 item slots a wavefront keeps in registers, and a second list (the rounds are numbered through both)
        features[1]["count"] = 200
        features.append({"name": "seen", "type": "interacted_with", "interaction": "view", "field": ["item.g3", "item.w9"], "field_order": ["g3", "w9"],
                         "scope": "session", "count": 200, "duration": "24h"})
    return {"features": features, "models": {"m": {"type": "lambdamart", "backend": {"type": "lightgbm", "iterations": 10}, "features": [f["name"] for f in features]}}}


def state(seed=25):
    rng = np.random.Generator(np.random.PCG64(seed))
    puts = []
    for i in range(N_ITEMS):
        if rng.random() < 0.06:
            continue   # an item without state
        puts.append(("double", f"item={i}/pop", float(rng.integers(0, 1000))))
        puts.append(("string_list", f"item={i}/prof_g3", [f"g{t}" for t in rng.integers(0, 3, int(rng.integers(0, 4)))]))
        puts.append(("string_list", f"item={i}/prof_v40", [f"v{t}" for t in rng.integers(0, 40, int(rng.integers(0, 13)))]))   # up to 12: past TOK_BATCH
        puts.append(("string_list", f"item={i}/prof_one", ["only"]))
        puts.append(("string_list", f"item={i}/prof_w9", [f"w{t}" for t in rng.integers(0, 9, int(rng.integers(0, 3)))]))
        if rng.random() < 0.9:
            puts.append(("double", f"item={i}/div_price", float(rng.integers(0, 500)) / 4))
        if rng.random() < 0.9:
            puts.append(("string_list", f"item={i}/div_g3", [f"g{t}" for t in rng.integers(0, 3, int(rng.integers(1, 4)))]))
        if rng.random() < 0.8:
            puts.append(("string_list", f"item={i}/div_v40", [f"v{t}" for t in rng.integers(0, 40, int(rng.integers(1, 13)))]))
        puts.append(("string", f"item={i}/div_one", "only"))
        puts.append(("double", f"item={i}/div_pop", float(rng.integers(0, 50))))
        puts.append(("double", f"item={i}/div_rank", float((i * 37) % 11) - 5.0))   # ties, +-0 (kind "nums": three numeric entries in one group)
        puts.append(("string_list", f"item={i}/seen_g3", [f"g{(i + t) % 3}" for t in range(i % 3)]))
        puts.append(("string_list", f"item={i}/seen_w9", [f"w{(i * 5 + t) % 9}" for t in range(i % 4)]))
        if rng.random() < 0.7:
            puts.append(("string_list", f"item={i}/div_w9", [f"w{t}" for t in rng.integers(0, 9, int(rng.integers(1, 3)))]))
        if rng.random() < 0.5:
            puts.append(("string", f"item={i}/div_z", f"z{int(rng.integers(0, 5))}"))
    for k in range(N_BARE):
        puts.append(("double", f"item=bare{k}/pop", float(k)))
        puts.append(("string_list", f"item=bare{k}/prof_v40", [f"v{k % 40}"]))
    for s, ln in SESSIONS.items():
        puts.append(("bounded_list", f"session={s}/prof_interactions", [str(x) for x in rng.integers(0, N_ITEMS, ln)]))
    for s, ln in (("s150", 150), ("s100", 100), ("s16", 16)):   # kind "lists": 150 clicks (tasks with k >= 128) and a second list of views
        if s == "s150":
            puts.append(("bounded_list", f"session={s}/prof_interactions", [str((k * 7) % N_ITEMS) for k in range(ln)]))
        puts.append(("bounded_list", f"session={s}/seen_interactions", [str((k * 11 + 3) % N_ITEMS) for k in range(ln if s != "s150" else 140)]))
    puts.append(("bounded_list", "session=srep/prof_interactions", ["7"] * 100))   # one item 100 times: counts, not keys, grow
    puts.append(("string_list", "item=7/prof_v40", ["v1", "v2", "v3"]))
    return puts


def request(name, session, n, seed, bare=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = rng.choice(N_ITEMS, size=n - bare, replace=False)
    items = [{"id": f"bare{k}"} for k in range(bare)] + [{"id": (str(x) if rng.random() >= 0.03 else f"unknown{x}")} for x in ids]
    return {"id": name, "timestamp": ranklens.TS, "user": "u", "session": session, "fields": [], "items": items}


REQUESTS = {
    "n1": ("s0", 1, 0), "n19": ("s1", 19, 0), "n20": ("s15", 20, 0), "n21": ("s16", 21, 0), "n63": ("s17", 63, 0), "n64": ("s64", 64, 0),
    "n65": ("s65", 65, 0), "n100": ("s100", 100, 0), "rep": ("srep", 100, 0), "lead1": ("s15", 70, 1), "lead5": ("s100", 70, 5),
    "lead64": ("s64", 100, 64), "a70": ("s100", 70, 0), "b70": ("s15", 70, 0), "c70": ("s0", 70, 0), "n130": ("s100", 130, 0),
    "l150": ("s150", 100, 0),
}
MAIN_BATCHES = [["n1", "n19", "n20"], ["n21", "n63", "n64"], ["n65", "n100", "rep"], ["lead1", "lead5", "lead64"]]
OTHER_BATCHES = [["n21", "n65", "lead64"], ["n100", "lead5", "n20"]]
LISTS_BATCHES = [["l150", "n100", "n21"]]


def build_world(kind):
    """the oracle's answers for every request of a config (computed once, never changed) and the forest"""
    cfg, puts = config(kind), state()
    names = [n for n in REQUESTS if n != "l150"] if kind == "main" else sorted({n for bt in (LISTS_BATCHES if kind == "lists" else OTHER_BATCHES) for n in bt})
    reqs = {n: request(n, REQUESTS[n][0], REQUESTS[n][1], 100 + i, REQUESTS[n][2]) for i, n in enumerate(REQUESTS) if n in names}
    orc = OracleBackend(cfg, "m")
    ranklens.load_state(orc, puts)
    mats = {k: orc.matrix(ev) for k, ev in reqs.items()}
    allm = np.concatenate(list(mats.values()))
    blob = synth.synthetic_lgbm_model(n_trees=40, n_features=allm.shape[1], quantiles=ranklens.column_quantiles(allm), missing="per_feature")
    orc.load_model(blob, 0)
    expected = {k: orc.rerank(ev) for k, ev in reqs.items()}
    orc.close()
    return {"cfg": cfg, "puts": puts, "reqs": reqs, "mats": mats, "blob": blob, "expected": expected}


_worlds = {}


def world(kind):
    if kind not in _worlds:
        _worlds[kind] = build_world(kind)
    return _worlds[kind]


def run_batch(hip, names, w, kernel, what, entry_bytes=None):
    """ranks the batch; results against the oracle bit for bit, status 0, the kernel and the table form that ran"""
    batch = hip.ranker.prepare("m", [w["reqs"][n] for n in names])
    try:
        batch.run(hip.booster)
        scores, order, _ = batch.fetch()
        info = batch.launch_info()
        print(what, names, info)
        assert (batch.status() == 0).all(), (what, batch.status())
        assert info["kernel"] == kernel and info["entry_bytes"] == (entry_bytes or (4 if kernel == PLAIN else 8)), (what, info)
        _, _, mat = batch.fetch(matrix=True)
        for r, n in enumerate(names):
            _, es, eo = w["expected"][n]
            lo, hi = batch.offsets[r], batch.offsets[r + 1]
            assert same(mat[lo:hi], w["mats"][n]), (what, r, n)
            assert same(scores[lo:hi], es) and order[lo:hi].tolist() == eo.tolist(), (what, r, n)
        return scores, order, mat
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


_default_form = []   # what the plain kernel with both switches at their defaults returned for MAIN_BATCHES (computed once, never changed)


def plain_kernel_results(hip, w, defs):
    extra = {"MRK_JIT_DEFINES": defs} if defs else {}
    set_switches(MRK_RANK_JIT="1", MRK_FUSED_SPLIT="1", **extra)      # a handful of requests made to take the plain kernel: two wavefronts
    return [run_batch(hip, bt, w, PLAIN, f"plain {defs}") for bt in MAIN_BATCHES]


# (a case per form: each compiles its own specialised kernel)
@pytest.mark.gpu
@pytest.mark.parametrize("defs", [None, "MRK_PRE_SIDE=0 MRK_PRE_SHARE=0", "MRK_PRE_SIDE=1 MRK_PRE_SHARE=1", "MRK_PRE_SIDE=0 MRK_PRE_SHARE=1", "interpreting"])
def test_all_lanes_prepass_gives_the_oracles_bytes_with_either_switch(defs, switches):
    w = world("main")
    hip = backend(w)
    try:
        if not _default_form:
            _default_form.extend(plain_kernel_results(hip, w, None))
        if defs == "interpreting":
            set_switches(MRK_RANK_JIT="0", MRK_FUSED_SPLIT="1")
            res = [run_batch(hip, bt, w, INTERPRETING, "interpreting", entry_bytes=8) for bt in MAIN_BATCHES]
        else:
            res = plain_kernel_results(hip, w, defs) if defs else _default_form
        for (s, o, m), (s0, o0, m0) in zip(res, _default_form):
            assert same(s, s0) and o.tolist() == o0.tolist() and same(m, m0), defs
    finally:
        hip.close()


@pytest.mark.gpu
def test_all_lanes_prepass_in_the_split_and_sliced_kernels(switches):
    w = world("main")
    hip = backend(w)
    try:
        set_switches(MRK_RANK_JIT="1")
        run_batch(hip, ["a70", "b70", "c70"], w, SPLIT, "3x70: op split")      # eight wavefronts: seven on the tasks
        run_batch(hip, ["n130"], w, SPLIT, "1x130: by its shape")
        set_switches(MRK_RANK_JIT="1", MRK_FUSED_SLICES="2", MRK_FUSED_SPLIT="1", MRK_FUSED_THREADS="128")
        run_batch(hip, ["n130"], w, SPLIT, "1x130: two slices of two wavefronts")
        set_switches(MRK_RANK_JIT="1", MRK_FUSED_SLICES="2", MRK_FUSED_SPLIT="1", MRK_FUSED_THREADS="64")
        run_batch(hip, ["n130"], w, SPLIT, "1x130: two slices of one wavefront")   # a lone wavefront: the sections one after the other
        set_switches(MRK_RANK_JIT="0")
        run_batch(hip, ["a70", "b70", "c70"], w, INTERPRETING, "3x70 interpreting", entry_bytes=8)
        run_batch(hip, ["n130"], w, INTERPRETING, "1x130 interpreting", entry_bytes=8)
    finally:
        hip.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["top3", "top64", "top65", "five", "single", "nums", "lists"])
def test_all_lanes_prepass_over_top_and_entry_counts(kind, switches):
    w = world(kind)
    hip = backend(w)
    batches = LISTS_BATCHES if kind == "lists" else OTHER_BATCHES
    try:
        extra = {"MRK_JIT_DEFINES": "MRK_PRE_SIDE=1 MRK_PRE_SHARE=1"} if kind == "lists" else {}   # (the claim counter across two lists)
        set_switches(MRK_RANK_JIT="1", MRK_FUSED_SPLIT="1", **extra)
        a = [run_batch(hip, bt, w, PLAIN, f"{kind} plain") for bt in batches]
        set_switches(MRK_RANK_JIT="0", MRK_FUSED_SPLIT="1")
        b = [run_batch(hip, bt, w, INTERPRETING, f"{kind} interpreting", entry_bytes=8) for bt in batches]
        for (s, o, m), (s0, o0, m0) in zip(a, b):
            assert same(s, s0) and o.tolist() == o0.tolist() and same(m, m0), kind
    finally:
        hip.close()


@pytest.mark.gpu
def test_all_lanes_prepass_on_wide_tables_after_token_id_2_pow_20(switches):
    w = world("main")
    # four lists of 262 200 new tokens in a table's column, on items no request asks for: the store's token ids pass 2^20
    junk = [("string_list", f"item=junk{k}/div_one", [f"j{k}_{i}" for i in range(262_200)]) for k in range(4)]
    hip = backend(w, junk)
    try:
        set_switches(MRK_RANK_JIT="1", MRK_FUSED_SPLIT="1")
        assert hip.ranker.column_distinct("div_one") == 4 * 262_200 + 1
        run_batch(hip, ["n65", "n100", "rep"], w, SPLIT, "token id >= 2^20: wide, two wavefronts")
    finally:
        hip.close()
