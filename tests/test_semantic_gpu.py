"""GPU: the semantic recommender's fit on the device (mrk_index_build_texts, mrk_index_vectors; csrc/capi_index.cpp,
knn_pool_pack_kernel in csrc/knn.hip).  An f32 encoder handle gives a text the same bits whatever batch it travels in, so every
stored row must have the bits of mrk_encoder_embed of that text ALONE, however the catalogue is cut into pieces; neighbours and
distance bits come from the numpy restatement (tests/knn_reference.py).  No tolerance anywhere except the fp16 handle's cosine.

Shapes: hidden 64 (16 groups of 4), truncation at 24 tokens, 150 rows = 2 blocks of 64 + 22; budgets 1 / 37 / 100 / default cut
the 2 345 tokens into 150 / ~70 / ~25 / 1 pieces whose boundaries fall inside the 64-row blocks."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import knn_reference as K
import metarank_amd as M
import semantic_cases as S
from metarank_amd import _native as N
from metarank_amd.encoder import HipEncoder
from metarank_amd.index import HipIndex

pytestmark = pytest.mark.gpu

ATOL_COS = 3e-3   # tests/test_encoder_gpu.py: what the fp16 path is held to against the fp32 graph
BUDGETS = [1, 37, 100, 0]


def f32bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def load(ctx, precision):
    return HipEncoder(open(os.path.join(S.GOLDEN, "encoder_tiny.onnx"), "rb").read(), open(os.path.join(S.GOLDEN, "tokenizer_tiny.json"), "rb").read(),
                      ctx=ctx, precision=precision)


@pytest.fixture(scope="module")
def enc(ctx):
    e = load(ctx, "f32")
    yield e
    e.close()


@pytest.fixture(scope="module")
def cat(enc):
    """the 150 texts, each text's embedding taken one text at a time (the reference of every test; never modified)"""
    ids, texts = S.catalogue()
    alone = np.concatenate([enc.embed([t]) for t in texts])
    alone.setflags(write=False)
    return ids, texts, alone


def assert_rows(ix, emb):
    """the stored rows are `emb` (float32), bit for bit, widened"""
    v = ix.vectors()
    assert v.dtype == np.float64 and v.shape == emb.shape
    assert np.array_equal(v.view(np.uint64), emb.astype(np.float64).view(np.uint64))
    assert np.array_equal(f32bits(v.astype(np.float32)), f32bits(emb))


def test_one_piece(ctx, enc):
    texts = S.FILMS
    ids = [f"m{i}" for i in range(len(texts))]
    emb = enc.embed(texts)
    a = HipIndex.fit_semantic(enc, ids, texts)
    b = HipIndex.build(ids, emb, ctx)
    assert a.info() == b.info() and a.info() == {"rows": 9, "cols": 64, "stored_elem_bytes": 4, "device_bytes": b.info()["device_bytes"]}
    assert_rows(a, emb)
    assert a.ids() == ids and a.row("m4") == 4
    for items in (["m0"], ["m3", "m4"]):
        r, d = a.lookup(items, len(texts))
        er, ed = K.lookup(ids, emb.astype(np.float64), items, len(texts))
        assert np.array_equal(r, er) and np.array_equal(K.bits(d), K.bits(ed))
    assert np.array_equal(a.vectors([8, 0, 8]).view(np.uint64), emb[[8, 0, 8]].astype(np.float64).view(np.uint64))
    assert a.vectors([]).shape == (0, 64)
    a.close()
    b.close()


@pytest.fixture
def window(request, monkeypatch):
    """both forms of the fit: windows of sequences in length order (the default) and input order"""
    monkeypatch.setenv("MRK_SEMANTIC_WINDOW", str(request.param))
    N.reload_switches()
    yield request.param
    monkeypatch.delenv("MRK_SEMANTIC_WINDOW")
    N.reload_switches()


@pytest.mark.parametrize("window", [4, 0], indirect=True)
@pytest.mark.parametrize("budget", BUDGETS)
def test_many_pieces_straddle_blocks(enc, cat, budget, window):
    ids, texts, alone = cat
    ix = HipIndex.fit_semantic(enc, ids, texts, max_tokens=budget)
    assert ix.info()["rows"] == 150 and ix.info()["cols"] == 64 and ix.info()["stored_elem_bytes"] == 4
    assert_rows(ix, alone)                       # ... and therefore identical across budgets
    table = alone.astype(np.float64)
    queries = table[[0, 70, 149]]
    rows, dist = ix.search(queries, 150)         # all 150: the norms of every row are right, the zero rows of the last block never come back
    for q in range(3):
        er, ed = K.search(table, queries[q], 150)
        assert len(rows[q]) == 150 and np.array_equal(rows[q], er) and np.array_equal(K.bits(dist[q]), K.bits(ed)), (budget, q)
    assert sorted(rows[0].tolist()) == list(range(150))
    rows, _ = ix.search(queries, 200)            # more than there are
    assert [len(r) for r in rows] == [150, 150, 150]
    ix.close()


def test_same_answers_as_the_existing_join(enc, cat):
    ids, texts, alone = cat
    a = HipIndex.fit_semantic(enc, ids, texts, max_tokens=37)
    b = HipIndex.from_encoder(enc, ids, texts)
    assert a.info() == b.info()
    assert np.array_equal(a.vectors().view(np.uint64), b.vectors().view(np.uint64))
    for items, count in ((["item-3"], 10), (["item-5", "item-70", "ghost"], 40), (["item-149"], 149)):
        ra, sa = a.recommend(items, count)
        rb, sb = b.recommend(items, count)
        er, es = K.recommend(ids, alone.astype(np.float64), items, count)
        assert np.array_equal(ra, rb) and np.array_equal(K.bits(sa), K.bits(sb))
        assert np.array_equal(ra, er) and np.array_equal(K.bits(sa), K.bits(es))
    a.close()
    b.close()


def test_fp16_handle(ctx, cat):
    ids, texts, alone = cat
    e16 = load(ctx, "f16")
    together = e16.embed(texts)
    one = HipIndex.fit_semantic(e16, ids, texts, max_tokens=1 << 20)    # one piece: the same launches as the one embed call
    assert_rows(one, together)
    one.close()
    cut = HipIndex.fit_semantic(e16, ids, texts, max_tokens=37)
    v = cut.vectors()
    w = alone.astype(np.float64)
    cos = (v * w).sum(axis=1) / np.sqrt((v * v).sum(axis=1) * (w * w).sum(axis=1))
    print("fp16 rows against f32 rows, max |cos - 1| =", float(np.abs(cos - 1.0).max()))
    assert np.abs(cos - 1.0).max() < ATOL_COS
    cut.close()
    e16.close()


def test_refusals(ctx, enc, cat):
    ids, texts, alone = cat
    L = N.lib()

    def raw(id_list, text_list, budget):
        pi = (C.c_char_p * len(id_list))(*[s if s is None else s.encode() for s in id_list])
        pt = (C.c_char_p * len(text_list))(*[s if s is None else s.encode() for s in text_list])
        out = C.c_void_p(1)
        rc = L.mrk_index_build_texts(ctx.handle, enc.handle, pi, pt, len(id_list), budget, C.byref(out))
        return rc, out.value, (L.mrk_last_error() or b"").decode()

    def good():
        ix = HipIndex.fit_semantic(enc, ids[:20], texts[:20], max_tokens=37)
        assert_rows(ix, alone[:20])
        ix.close()

    rc, out, msg = raw(ids[:6], texts[:3] + [None] + texts[4:6], 0)
    assert rc == N.ERR_INVALID_ARG and not out and "row 3" in msg and "text" in msg
    good()
    rc, out, msg = raw(ids[:3] + [None] + ids[4:6], texts[:6], 0)
    assert rc == N.ERR_INVALID_ARG and not out and "row 3" in msg
    good()
    rc, out, msg = raw(ids[:4] + [ids[1]], texts[:5], 0)
    assert rc == N.ERR_INVALID_ARG and not out and "stored twice" in msg and "row 4" in msg
    with pytest.raises(M.MrkError) as e:                 # ... the message of mrk_index_build for the same ids
        HipIndex.build(ids[:4] + [ids[1]], alone[:5], ctx)
    assert e.value.message == msg
    good()
    rc, out, msg = raw(ids[:5], texts[:5], -1)
    assert rc == N.ERR_INVALID_ARG and not out and "max_tokens" in msg
    good()
    other = M.Context(0)
    out = C.c_void_p(1)
    pi = (C.c_char_p * 1)(b"a")
    assert L.mrk_index_build_texts(other.handle, enc.handle, pi, pi, 1, 0, C.byref(out)) == N.ERR_INVALID_ARG and not out.value
    assert b"another context" in L.mrk_last_error()
    other.close()
    good()
    ix = HipIndex.fit_semantic(enc, ids, texts)
    with pytest.raises(M.MrkError) as e:
        ix.vectors([0, 150])
    assert e.value.status == N.ERR_INVALID_ARG and "150" in e.value.message
    with pytest.raises(M.MrkError) as e:
        ix.vectors([-1])
    assert e.value.status == N.ERR_INVALID_ARG
    assert_rows(ix, alone)
    ix.close()
    empty = HipIndex.fit_semantic(enc, [], [])
    assert empty.info()["rows"] == 0 and empty.info()["cols"] == 64 and empty.vectors().shape == (0, 64)
    assert len(empty.lookup(["a"], 3)[0]) == 0
    empty.close()
    good()


def test_the_handle_is_shared_not_held(enc, cat):
    ids, texts, alone = cat
    quiet = enc.embed(["star wars"])
    got, errors = [], []

    def caller():
        try:
            for _ in range(50):
                got.append(enc.embed(["star wars"]))
        except Exception as e:     # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=caller)
    t.start()
    ix = HipIndex.fit_semantic(enc, ids, texts, max_tokens=1)
    t.join()
    assert not errors and len(got) == 50
    for g in got:
        assert np.array_equal(f32bits(g), f32bits(quiet))
    assert_rows(ix, alone)
    ix.close()


def test_many_sequences_in_one_piece(enc):
    n = 200
    ids = [str(i) for i in range(n)]
    ix = HipIndex.fit_semantic(enc, ids, [""] * n, max_tokens=1 << 20)
    one = enc.embed([""])
    assert_rows(ix, np.repeat(one, n, axis=0))
    rows, dist = ix.search(one.astype(np.float64), n)
    assert rows[0].tolist() == list(range(n)) and len(set(K.bits(dist[0]).tolist())) == 1     # ties by ascending row
    er, ed = K.search(np.repeat(one, n, axis=0).astype(np.float64), one[0].astype(np.float64), n)
    assert np.array_equal(rows[0], er) and np.array_equal(K.bits(dist[0]), K.bits(ed))
    ix.close()
