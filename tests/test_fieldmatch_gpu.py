"""GPU: field_match term / ngram / bm25 computed on the device ("match": "device") - the matrix columns of mrk_rank and of the
batch path compared BIT FOR BIT with the line-by-line transcription of the reference's matchers (tests/fieldmatch_reference.py)
over every kind of item state and query, through every assembly kernel variant and the serving queue."""
import os

import numpy as np
import pytest

import fieldmatch_reference as R
import metarank_amd as M
from metarank_amd import _native as N
from metarank_amd.ranker import HipRanker
from metarank_amd.request import F_STRING_LIST, Request
from workloads import ranklens, synth

pytestmark = pytest.mark.gpu

ENV = ("MRK_RANK_FUSED", "MRK_RANK_CELLS", "MRK_RANK_JIT", "MRK_RANK_ONE", "MRK_JIT_SIG")
FIELDS = {"m_term": "title", "m_ngram": "desc", "m_bm25": "tags"}
METHOD = {"m_term": "term", "m_ngram": "ngram", "m_bm25": "bm25"}

VOCAB = sorted([f"w{i:03d}" for i in range(400)] + ["é", "中", "�", "\U0001f600", "\U00010000x"], key=R.utf16_key)
UNKNOWN = sorted([f"zz-never-stored-{i}" for i in range(130)], key=R.utf16_key)   # tokens the store never interns
DIC = {"language": "en", "fields": ["tags"], "docs": 50, "avgdl": 11.5,
       # w000 has gtf > docs (a negative idf); most tokens are missing from the dictionary (gtf 0)
       "termfreq": dict({"w000": 80, "w001": 50, "w002": 1, "é": 7, "\U0001f600": 3}, **{f"w{i:03d}": 1 + i % 37 for i in range(10, 200, 3)})}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def config():
    def fm(name, method):
        return {"name": name, "type": "field_match", "match": "device", "rankingField": "ranking.query", "itemField": "item." + FIELDS[name], "method": method}
    feats = [{"name": "pop", "type": "number", "scope": "item", "source": "item.pop"},
             fm("m_term", {"type": "term", "language": "en"}), fm("m_ngram", {"type": "ngram", "language": "en", "n": 3}),
             fm("m_bm25", {"type": "bm25", "language": "en", "termFreq": "tf.json"})]
    return {"features": feats, "models": {"xgboost": {"type": "lambdamart", "features": [f["name"] for f in feats]}}}


def pick(rng, n, pool=VOCAB):
    return sorted((pool[i] for i in rng.choice(len(pool), size=n, replace=False)), key=R.utf16_key)


def make_items(heap_cap):
    """id -> {field: list | "a string" | None}: every kind of state, lists on both sides of the record's inline heap"""
    rng = np.random.Generator(np.random.PCG64(7))
    inline = heap_cap // 4   # tokens the inline heap holds (taken from the store)
    items = {}
    sizes = [1, 2, 63, 64, 65, 200] + sorted({max(inline - 1, 1), inline, inline + 1})
    for k, n in enumerate(sizes):
        items[f"len{n}-{k}"] = {"title": pick(rng, n), "desc": pick(rng, max(1, n // 2)), "tags": pick(rng, n)}
    for k in range(12):      # short lists over the head of the vocabulary: some match part of a query, some none of it
        items[f"short{k}"] = {f: pick(rng, int(rng.integers(1, 9)), VOCAB[:40 if k % 2 else 400]) for f in ("title", "desc", "tags")}
    items["all"] = {"title": list(VOCAB), "desc": list(VOCAB[:128]), "tags": list(VOCAB[:64])}
    items["empty"] = {"title": [], "desc": [], "tags": []}
    items["nostate"] = {"title": None, "desc": None, "tags": None}
    items["othertype"] = {"title": "a string", "desc": "a string", "tags": "a string"}
    items["mixed"] = {"title": pick(rng, 5), "desc": None, "tags": []}
    for k in range(8):
        items[f"mid{k}"] = {f: pick(rng, int(rng.integers(9, 40))) for f in ("title", "desc", "tags")}
    return items


def load_items(ranker, items):
    for iid, st in items.items():
        ranker.put_double(f"item={iid}/pop", float(len(iid)))
        for name, field in FIELDS.items():
            v = st[field]
            if isinstance(v, str):
                ranker.put_string(f"item={iid}/{name}_{field}", v)
            elif v is not None:
                ranker.put_string_list(f"item={iid}/{name}_{field}", v)


def event(rid, ids, queries):
    """queries: {feature: token list | None}; None = no field"""
    fields = [{"name": "__tokens:" + name, "value": q} for name, q in queries.items() if q is not None]
    return {"id": rid, "timestamp": ranklens.TS, "user": "u", "session": "s", "fields": fields, "items": [{"id": i} for i in ids]}


def request(ev):
    rq = Request(ev)
    for i in range(rq.c.n_fields):   # an empty query is the empty STRING list, not the absent-field path
        assert rq.c.fields[i].type == F_STRING_LIST, rq.c.fields[i].name
    return rq


def expected(items, ids, queries):
    cols = []
    for name, field in FIELDS.items():
        states = [items[i][field] if i in items and isinstance(items[i][field], list) else None for i in ids]
        cols.append(R.column(METHOD[name], queries.get(name), states, DIC))
    pop = [float(len(i)) if i in items else float("nan") for i in ids]
    return np.array([pop] + cols, dtype=np.float64).T


def query_cases():
    rng = np.random.Generator(np.random.PCG64(3))
    head = VOCAB[:40]
    q = {"absent": None, "empty": [], "one": [VOCAB[17]], "known+unknown": sorted([VOCAB[5], UNKNOWN[0]], key=R.utf16_key),
         "63": pick(rng, 63), "64": pick(rng, 64, head + VOCAB[200:260]), "128": pick(rng, 128), "unicode": ["w003", "é", "中", "\U0001f600", "�"],
         "all-unknown": UNKNOWN[:3]}
    assert all(R.strictly_ascending(v) for v in q.values() if v)
    return q


class Env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in ENV}
        os.environ.update(self.kw)
        M.reload_switches()

    def __exit__(self, *a):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        M.reload_switches()


class Ranker(HipRanker):
    """a HipRanker on a context of its own, closed with it"""

    def __init__(self, cfg):
        self._ctx = M.Context(0)
        super().__init__(cfg, self._ctx)

    def close(self):
        super().close()
        self._ctx.close()


@pytest.fixture(scope="module")
def world():
    ranker = Ranker(config())
    info = ranker.store_info(1)
    items = make_items(info["heap_cap"])
    load_items(ranker, items)
    after = ranker.store_info(1)
    assert info["heap_cap"] >= 4 and after["tok_pool"] > info["tok_pool"]   # both homes of a list are in play
    ranker.bind_termfreq("m_bm25", DIC)
    ids = list(items) + ["nobody-1", "nobody-2"]
    yield ranker, items, ids
    ranker.close()


def sized(ids, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return list(ids) * (n // len(ids)) + [ids[i] for i in rng.permutation(len(ids))[:n % len(ids)]] if n >= len(ids) else [ids[i] for i in rng.permutation(len(ids))[:n]]


def test_every_state_and_query_bit_for_bit(world):
    ranker, items, ids = world
    with Env(MRK_RANK_JIT="0"):
        for name, q in query_cases().items():
            queries = {"m_term": q, "m_ngram": q, "m_bm25": None if q is None else q[:64]}
            for n in (1, 100, 300) if name in ("64", "absent") else (len(ids),):
                use = sized(ids, n, 5) if n != len(ids) else ids
                mat, _, _ = ranker.rerank("xgboost", request(event(f"r-{name}-{n}", use, queries)), None, explain=True)
                want = expected(items, use, queries)
                assert mat.shape == want.shape and (bits(mat) == bits(want)).all(), (name, n, np.argwhere(bits(mat) != bits(want))[:5])
        # the cases are not vacuous: hits, misses, partial matches, a negative bm25 term
        q = query_cases()["64"]
        want = expected(items, ids, {"m_term": q, "m_ngram": q, "m_bm25": ["w000"] + [t for t in q if t != "w000"][:63]})
        assert (want[:, 1] > 0).any() and (want[:, 1] == 0).any() and ((want[:, 1] > 0) & (want[:, 1] < 1)).any()
    mat, _, _ = ranker.rerank("xgboost", request(event("neg", ids, {"m_bm25": ["w000"]})), None, explain=True)
    want = expected(items, ids, {"m_bm25": ["w000"]})
    assert (want[:, 3] < 0).any() and (bits(mat) == bits(want)).all()
    full = {"m_term": list(VOCAB[:128]), "m_ngram": list(VOCAB[:128]), "m_bm25": list(VOCAB[:64])}
    mat, _, _ = ranker.rerank("xgboost", request(event("full", ["all"], full)), None, explain=True)
    assert mat[0, 2] == 1.0 and (bits(mat) == bits(expected(items, ["all"], full))).all()


def test_refused_inputs(world):
    ranker, items, ids = world
    def status(queries):
        with pytest.raises(M.MrkError) as e:
            ranker.rerank("xgboost", request(event("bad", ids[:3], queries)), None, explain=True)
        return e.value.status
    assert status({"m_term": list(VOCAB[:129])}) == N.ERR_UNSUPPORTED      # never truncated
    assert status({"m_ngram": list(VOCAB[:129])}) == N.ERR_UNSUPPORTED
    assert status({"m_bm25": list(VOCAB[:65])}) == N.ERR_UNSUPPORTED
    assert status({"m_term": ["b", "a"]}) == N.ERR_INVALID_ARG
    assert status({"m_bm25": ["a", "a"]}) == N.ERR_INVALID_ARG
    assert status({"m_term": ["�", "\U0001f600"]}) == N.ERR_INVALID_ARG       # ascending in UTF-8 bytes, descending in UTF-16
    for bad in (["b", "a"], ["a", "a"], ["�", "\U0001f600"]):
        with pytest.raises(M.MrkError) as e:
            ranker.put_string_list("item=len1-0/m_term_title", bad)
        assert e.value.status == N.ERR_UNSUPPORTED
    from oracle import codec
    with pytest.raises(M.MrkError) as e:
        ranker.put_binary(codec.feature_value("string_list", "item=len1-0/m_term_title", ["b", "a"]))
    assert e.value.status == N.ERR_UNSUPPORTED
    assert ranker.put_binary(codec.feature_value("string_list", "item=len1-0/m_term_title", items["len1-0"]["title"])) == 1
    ranker.put_string_list("item=len1-0/pop", ["b", "a"])   # a column no matcher reads takes any list
    ranker.put_double("item=len1-0/pop", float(len("len1-0")))
    # the refused puts changed nothing
    q = {"m_term": items["len1-0"]["title"]}
    mat, _, _ = ranker.rerank("xgboost", request(event("after", ["len1-0"], q)), None, explain=True)
    assert mat[0, 1] == 1.0
    # dictionaries the reference cannot have written
    for dic in (dict(DIC, docs=-1), dict(DIC, avgdl=0.0), dict(DIC, avgdl=-1.0), b'{"language": "en"'):
        with pytest.raises(M.MrkError):
            ranker.bind_termfreq("m_bm25", dic)
    with pytest.raises(M.MrkError) as e:
        ranker.bind_termfreq("m_term", DIC)
    assert e.value.status == N.ERR_UNSUPPORTED
    with pytest.raises(M.MrkError) as e:
        ranker.bind_termfreq("nope", DIC)
    assert e.value.status == N.ERR_NOT_FOUND


def test_bm25_without_a_dictionary_is_an_error():
    ranker = Ranker(config())
    try:
        ranker.put_string_list("item=a/m_bm25_tags", ["x"])
        with pytest.raises(M.MrkError) as e:
            ranker.rerank("xgboost", request(event("r", ["a"], {"m_bm25": ["x"]})), None, explain=True)
        assert "bind_termfreq" in e.value.message
        ranker.bind_termfreq("m_bm25", DIC)
        mat, _, _ = ranker.rerank("xgboost", request(event("r", ["a"], {"m_bm25": ["x"]})), None, explain=True)
        assert bits(mat[0, 3]) == bits(R.bm25_score(["x"], ["x"], DIC))
    finally:
        ranker.close()


def test_batch_kernel_variants_and_the_serving_queue_agree(world):
    """five requests with five different queries (one without) through every assembly path: identical bytes, the reference's;
    a forest that splits on the match columns: scores = Booster.predict(matrix), order = the stable descending sort"""
    from oracle.assembly import sort_order

    ranker, items, ids = world
    qc = query_cases()
    qs = [{"m_term": qc["64"], "m_ngram": qc["63"], "m_bm25": qc["64"]}, {"m_term": None, "m_ngram": None, "m_bm25": None},
          {"m_term": qc["128"], "m_ngram": qc["one"], "m_bm25": qc["unicode"]}, {"m_term": qc["known+unknown"], "m_ngram": qc["128"], "m_bm25": ["w000", "w001", "w002"]},
          {"m_term": qc["unicode"], "m_ngram": [], "m_bm25": qc["63"]}]
    sizes = [100, 1, 300, len(ids), 37]
    evs = [event(f"b{r}", sized(ids, sizes[r], 20 + r), qs[r]) for r in range(5)]
    want = np.concatenate([expected(items, [it["id"] for it in ev["items"]], qs[r]) for r, ev in enumerate(evs)])
    quant = ranklens.column_quantiles(np.nan_to_num(want))
    booster = ranker.load_model(synth.synthetic_xgb_model(n_trees=40, n_features=4, depth=4, quantiles=quant), 1)
    reqs = [request(ev) for ev in evs]
    first = None
    for fused, cells, jit, one in (("1", "1", "require", "1"), ("1", "1", "0", "1"), ("1", "0", "0", "1"), ("0", "1", "0", "1"), ("0", "0", "0", "1"), ("1", "1", "0", "0")):
        with Env(MRK_RANK_FUSED=fused, MRK_RANK_CELLS=cells, MRK_RANK_JIT=jit, MRK_RANK_ONE=one):
            batch = ranker.prepare("xgboost", reqs)
            batch.run(booster)
            scores, order, mat = batch.fetch(matrix=True)
            assert (batch.status() == 0).all()
            assert (bits(mat) == bits(want)).all(), (fused, cells, jit, one)
            if first is None:
                assert ranker.kernel_keys("xgboost"), "MRK_RANK_JIT=require ran without a specialised kernel"
                first = (scores.copy(), order.copy())
                assert (bits(scores) == bits(booster.predict(mat))).all()
                for r in range(5):
                    lo, hi = batch.offsets[r], batch.offsets[r + 1]
                    assert order[lo:hi].tolist() == sort_order(scores[lo:hi]).tolist()
            assert (bits(scores) == bits(first[0])).all() and (order == first[1]).all(), (fused, cells, jit, one)
            # single requests (the one-launch kernel when it is on); interpreting kernels only: one compile is enough
            for r in (0, 1, 4) if jit == "0" else ():
                m1, s1, o1 = ranker.rerank("xgboost", reqs[r], booster, explain=True)
                lo, hi = batch.offsets[r], batch.offsets[r + 1]
                assert (bits(m1) == bits(want[lo:hi])).all() and (bits(s1) == bits(first[0][lo:hi])).all() and (o1 == first[1][lo:hi]).all()
            batch.close()
    with Env(MRK_RANK_JIT="0"):
        srv = ranker.serve("xgboost", booster)
        try:
            for r in range(5):
                s, o = srv.rerank(reqs[r])
                lo, hi = int(np.sum(sizes[:r])), int(np.sum(sizes[:r + 1]))
                assert (bits(s) == bits(first[0][lo:hi])).all() and (o == first[1][lo:hi]).all(), r
            assert srv.stats()["queue"] >= 1
        finally:
            srv.close()


def test_ranklens_columns_do_not_move():
    """the stock Ranklens model with two match features appended: its 24 columns are bit-identical, the two new ones the reference's"""
    n_items, n_sess = 400, 40
    base = ranklens.ranklens_config()
    ext = ranklens.ranklens_config()
    for name, field, method in (("t_term", "title", {"type": "term", "language": "en"}), ("t_bm25", "title", {"type": "bm25", "language": "en", "termFreq": "tf"})):
        ext["features"].append({"name": name, "type": "field_match", "match": "device", "rankingField": "ranking.query", "itemField": "item." + field, "method": method})
        ext["models"]["xgboost"]["features"].append(name)
    a, b = Ranker(base), Ranker(ext)
    try:
        puts = list(ranklens.generate_state(n_items, n_sess))
        ranklens.load_state(a, puts)
        ranklens.load_state(b, puts)
        rng = np.random.Generator(np.random.PCG64(9))
        lists = {str(i): pick(rng, int(rng.integers(0, 12)), VOCAB[:60]) for i in range(0, n_items, 2)}
        for iid, toks in lists.items():
            b.put_string_list(f"item={iid}/t_term_title", toks)
            b.put_string_list(f"item={iid}/t_bm25_title", toks)
        b.bind_termfreq("t_bm25", DIC)
        assert a.dim("xgboost") == 24 and b.dim("xgboost") == 26
        q = pick(rng, 9, VOCAB[:60])
        for ev in ranklens.generate_requests(4, 60, n_items, n_sess, seed=31):
            ev2 = dict(ev, fields=[{"name": "__tokens:t_term", "value": q}, {"name": "__tokens:t_bm25", "value": q}])
            with Env(MRK_RANK_JIT="0"):
                ma, _, _ = a.rerank("xgboost", ev, None, explain=True)
                mb, _, _ = b.rerank("xgboost", ev2, None, explain=True)
            assert (bits(ma) == bits(mb[:, :24])).all() and not np.isnan(ma).all()
            states = [lists.get(it["id"]) for it in ev["items"]]
            assert (bits(mb[:, 24]) == bits(R.column("term", q, states))).all()
            assert (bits(mb[:, 25]) == bits(R.column("bm25", q, states, DIC))).all()
    finally:
        a.close()
        b.close()
