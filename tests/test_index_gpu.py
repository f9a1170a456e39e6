"""GPU: the similar-items index (mrk_index_*, csrc/knn.hip) against the numpy restatement of the spec
(tests/knn_reference.py).  Rows and the bit patterns of the distances must be identical; there is no tolerance anywhere (a NaN
compares by java.lang.Double.doubleToLongBits' canonical pattern).

Shapes sit on the edges the kernels have: 64 rows per wavefront, 256 per workgroup of the scan, groups of 4 floats / 2
doubles per load, 4 096 rows per segment of the selection (one pass below, two passes above), lists of 512 / 1 024 / 2 048
pairs, 64 queries per launch."""
import os

import numpy as np
import pytest

import knn_reference as K
import metarank_amd as M
from metarank_amd import _native as N
from metarank_amd.index import HipIndex

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def ids_of(rows):
    return [str(i) for i in range(rows)]


def assert_search(ix, table, queries, n):
    rows, dist = ix.search(queries, n)
    assert len(rows) == len(queries)
    for q in range(len(queries)):
        er, ed = K.search(table, queries[q], n)
        assert np.array_equal(rows[q], er), (q, n, rows[q][:8], er[:8])
        assert np.array_equal(K.bits(dist[q]), K.bits(ed)), (q, n)


SHAPES = [(1, 1), (63, 3), (64, 100), (65, 384), (255, 3), (256, 1), (257, 100), (513, 384), (4095, 3), (4096, 5), (4097, 100), (8200, 2)]


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_shapes_both_widths(ctx, rows, cols):
    rng = np.random.default_rng(rows * 131 + cols)
    t64 = rng.normal(size=(rows, cols))
    t32 = t64.astype(np.float32)
    queries = np.stack([t64[rows // 2], rng.normal(size=cols), t32[0].astype(np.float64)])
    ns = sorted({1, max(rows - 1, 1), rows, rows + 5} if rows + 5 <= 2048 else {1, 10, 513, 2048})
    for table, width in ((t64, 8), (t32, 4)):
        ix = HipIndex.build(ids_of(rows), table, ctx)
        assert ix.info()["stored_elem_bytes"] == width and ix.info()["rows"] == rows and ix.info()["cols"] == cols
        for n in ns:
            assert_search(ix, table.astype(np.float64), queries, n)
        ix.close()


def test_reference_1000_x_100(ctx):
    """HnswJavaIndexTest.scala:13-22: 1000 x 100 uniform doubles, lookup of item "75", n = 10 -> 10 results; here the first is row
    75 itself at the distance the restatement gives, and the other nine are the true neighbours"""
    rng = np.random.default_rng(75)
    t = rng.random(size=(1000, 100))
    ix = HipIndex.build(ids_of(1000), t, ctx)
    rows, dist = ix.lookup(["75"], 10)
    er, ed = K.lookup(ids_of(1000), t, ["75"], 10)
    assert len(rows) == 10 and rows[0] == 75
    assert np.array_equal(rows, er) and np.array_equal(K.bits(dist), K.bits(ed))
    assert ix.ids(rows[:2]) == ["75", str(er[1])] and ix.row("75") == 75 and ix.row("nope") == -1
    ix.close()


def test_limits(ctx):
    t = np.random.default_rng(1).normal(size=(3000, 2))
    ix = HipIndex.build(ids_of(3000), t, ctx)
    assert_search(ix, t, t[:1], 2048)
    with pytest.raises(M.MrkError) as e:
        ix.search(t[:1], 2049)
    assert e.value.status == N.ERR_INVALID_ARG and "n + n_items <= 2048" in e.value.message
    with pytest.raises(M.MrkError) as e:
        ix.lookup(["1", "2"], 2047)
    assert e.value.status == N.ERR_INVALID_ARG and "n + n_items <= 2048" in e.value.message
    with pytest.raises(M.MrkError) as e:
        ix.recommend(["1", "2"], 2047)
    assert e.value.status == N.ERR_INVALID_ARG and "2048" in e.value.message
    r, d = ix.lookup(["1", "2"], 2046)
    er, ed = K.lookup(ids_of(3000), t, ["1", "2"], 2046)
    assert np.array_equal(r, er) and np.array_equal(K.bits(d), K.bits(ed))
    ix.close()
    for cols in (0, 4097):
        with pytest.raises(M.MrkError) as e:
            HipIndex.build(["a"], np.zeros((1, cols)), ctx)
        assert e.value.status == N.ERR_INVALID_ARG and "1 <= cols <= 4096" in e.value.message
    with pytest.raises(M.MrkError) as e:
        HipIndex.build(["a", "a"], np.zeros((2, 2)), ctx)
    assert e.value.status == N.ERR_INVALID_ARG


def test_ties_and_specials(ctx):
    rng = np.random.default_rng(9)
    base = rng.normal(size=(150, 7))
    t = np.repeat(base, 3, axis=0)                 # every vector three times: equal distances by ascending row
    t = np.concatenate([t, base[:5] * 3.0, base[:5] * 1e-3, np.zeros((3, 7)), np.full((1, 7), -0.0), np.zeros((2, 7))])
    t[7] = 0.0                                     # a zero vector among the early rows
    t = np.concatenate([t, np.full((2, 7), 1e-160), np.full((2, 7), 1e150), np.full((1, 7), -1e150)])   # norms underflow / overflow
    rows = len(t)
    ix = HipIndex.build(ids_of(rows), t, ctx)
    queries = np.stack([base[0], base[3], np.zeros(7), np.full(7, -0.0), np.full(7, 1e-160), np.full(7, 1e150), base[1] * 1e-158])
    for n in (1, 4, 12, rows):
        assert_search(ix, t, queries, n)
    r, d = ix.search(base[0], rows)
    at = r[0].tolist().index(0)
    assert r[0].tolist()[at:at + 3] == [0, 1, 2] and len(set(K.bits(d[0])[at:at + 3].tolist())) == 1   # the three copies of the query: one distance, by row
    nan_rows = r[0][np.isnan(d[0])]
    assert len(nan_rows) >= 7 and nan_rows.tolist() == sorted(nan_rows.tolist()) and np.isnan(d[0][-1])   # NaN last, by row
    ix.close()


def test_float32_and_float64_input_give_the_same_bits(ctx):
    rng = np.random.default_rng(4)
    t32 = rng.normal(size=(700, 33)).astype(np.float32)
    t32[5, :4] = [-0.0, np.float32(1e-40), np.finfo(np.float32).tiny / 4, 0.0]      # float denormals are stored as they are
    t64 = t32.astype(np.float64)
    queries = np.stack([t64[5], rng.normal(size=33)])
    a, b = HipIndex.build(ids_of(700), t32, ctx), HipIndex.build(ids_of(700), t64, ctx)
    assert a.info()["stored_elem_bytes"] == 4 and b.info()["stored_elem_bytes"] == 4
    t64b = t64.copy()
    t64b[699, 32] = 0.1                                                              # one value that does not round-trip
    c = HipIndex.build(ids_of(700), t64b, ctx)
    assert c.info()["stored_elem_bytes"] == 8 and c.info()["device_bytes"] > a.info()["device_bytes"]
    ra, da = a.search(queries, 700)
    rb, db = b.search(queries, 700)
    for q in range(2):
        assert np.array_equal(ra[q], rb[q]) and np.array_equal(K.bits(da[q]), K.bits(db[q]))
    assert_search(a, t64, queries, 700)
    assert_search(c, t64b, queries, 700)
    # the f64 table agrees with the f32 one on every row the changed value does not touch
    rc, dc = c.search(queries, 700)
    same = ra[0] != 699
    assert np.array_equal(K.bits(da[0][same]), K.bits(dc[0][rc[0] != 699]))
    for ix in (a, b, c):
        ix.close()


def test_batch_invariance_and_chunking(ctx):
    rng = np.random.default_rng(6)
    t = rng.normal(size=(1500, 19))
    ix = HipIndex.build(ids_of(1500), t, ctx)
    queries = rng.normal(size=(70, 19))               # one launch takes 64
    alone = [ix.search(queries[q], 25) for q in range(70)]
    for size in (5, 17, 70):
        rows, dist = ix.search(queries[:size], 25)
        for q in range(size):
            assert np.array_equal(rows[q], alone[q][0][0]) and np.array_equal(K.bits(dist[q]), K.bits(alone[q][1][0])), (size, q)
    assert_search(ix, t, queries[[0, 63, 64, 69]], 25)
    r, d = ix.search(np.zeros((0, 19)), 5)
    assert r == [] and d == []
    assert [len(x) for x in ix.search(queries[:2], 0)[0]] == [0, 0]
    ix.close()


def test_lookup(ctx):
    rng = np.random.default_rng(8)
    t = rng.normal(size=(300, 10))
    ids = [f"item-{i}" for i in range(300)]
    ix = HipIndex.build(ids, t, ctx)
    cases = [["item-7"], ["item-7", "item-9", "item-200"], ["item-7", "item-7", "item-9"], ["item-7", "ghost", "item-9", "???"], ["ghost", "item-9"],
             ["ghost"], ["ghost", "spectre"], []]
    for items in cases:
        for n in (1, 6, 300):
            r, d = ix.lookup(items, n)
            er, ed = K.lookup(ids, t, items, n)
            assert np.array_equal(r, er) and np.array_equal(K.bits(d), K.bits(ed)), (items, n)
    assert len(ix.lookup(["ghost", "spectre"], 5)[0]) == 0 and len(ix.lookup([], 5)[0]) == 0
    assert ix.lookup(["item-7"], 1)[0].tolist() == [7]
    assert ix.ids([0, 299]) == ["item-0", "item-299"]
    ix.close()


def test_recommend(ctx):
    rng = np.random.default_rng(10)
    t = rng.normal(size=(120, 6))
    ids = [f"p{i}" for i in range(120)]
    ix = HipIndex.build(ids, t, ctx)
    for items, count in ((["p3"], 5), (["p3", "p40", "p3"], 7), (["p3", "ghost"], 4), (["p1"], 200), (["p1", "p2"], 119)):
        r, s = ix.recommend(items, count)
        er, es = K.recommend(ids, t, items, count)
        assert np.array_equal(r, er) and np.array_equal(K.bits(s), K.bits(es)), (items, count)
        assert not set(ids[i] for i in r) & set(items)                       # the filter
        assert len(r) == min(count, 120 - len(set(items) & set(ids)))        # count larger than what is left
        assert np.all(np.diff(s) <= 0)                                       # farthest first
    lr, ld = ix.lookup(["p3"], 6)
    r, s = ix.recommend(["p3"], 5)
    assert lr[0] == 3 and r.tolist() == lr[1:][::-1].tolist()                # the nearest five, reversed
    with pytest.raises(M.MrkError) as e:
        ix.recommend([], 5)
    assert e.value.status == N.ERR_INVALID_ARG and "non-empty" in e.value.message
    with pytest.raises(M.MrkError) as e:
        ix.recommend(["ghost"], 5)
    assert e.value.status == N.ERR_NOT_FOUND
    ix.close()
    one = HipIndex.build(["only"], np.ones((1, 4)), ctx)
    with pytest.raises(M.MrkError) as e:
        one.recommend(["only"], 3)
    assert e.value.status == N.ERR_NOT_FOUND and "empty response from the recommender" in e.value.message
    one.close()


def test_from_encoder(ctx):
    from metarank_amd.encoder import HipEncoder

    enc = HipEncoder(open(os.path.join(GOLDEN, "encoder_tiny.onnx"), "rb").read(), open(os.path.join(GOLDEN, "tokenizer_tiny.json"), "rb").read(), ctx=ctx)
    texts = ["star wars", "the empire strikes back", "return of the jedi", "alien", "aliens", "blade runner", "the matrix", "matrix reloaded", "dune"]
    ids = [f"m{i}" for i in range(len(texts))]
    a = HipIndex.from_encoder(enc, ids, texts)
    emb = enc.embed(texts)
    b = HipIndex.build(ids, emb, ctx)
    assert emb.dtype == np.float32 and a.info() == b.info() and a.info()["stored_elem_bytes"] == 4 and a.info()["cols"] == enc.dim
    for items in (["m0"], ["m3", "m4"]):
        ra, da = a.lookup(items, len(texts))
        rb, db = b.lookup(items, len(texts))
        er, ed = K.lookup(ids, emb.astype(np.float64), items, len(texts))
        assert np.array_equal(ra, rb) and np.array_equal(K.bits(da), K.bits(db))
        assert np.array_equal(ra, er) and np.array_equal(K.bits(da), K.bits(ed))
    a.close()
    b.close()
    enc.close()
