"""Host-side mirror of the reference's KnnIndexReader / KnnIndexWriter for the device index.

Reference interfaces (ml/recommend/embedding/KnnIndex.scala:10-19, HnswJavaIndex.scala:23-87, MFRecommender.scala:66-80):
    KnnIndexWriter.write(EmbeddingMap(ids, embeddings, rows, cols)): KnnIndexReader
    KnnIndexReader.lookup(items: List[ItemId], n: Int): List[ItemScore]
    EmbeddingSimilarityModel.predict(RecommendRequest(count, items)): Response, ordered by Recommender.recommend
`HipIndex.build(ids, values)` is the drop-in for HnswIndexWriter.write; the scan of the table and the selection of the
nearest rows happen in libmrk_hip.so (csrc/knn.hip) and are exact - there is no CPU path and no approximation.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from .booster import Context, default_context


def _strs(vals):
    bs = [v.encode("utf-8", "surrogatepass") if isinstance(v, str) else v for v in vals]
    return (C.c_char_p * max(len(bs), 1))(*bs), bs


class HipIndex:
    def __init__(self, handle, ctx: Context):
        self._h = handle
        self.ctx = ctx

    @classmethod
    def build(cls, ids, values, ctx: Context | None = None) -> "HipIndex":
        """mrk_index_build: `values` is rows x cols, float32 or float64 (anything else is converted to float64)"""
        ctx = ctx or default_context()
        x = np.asarray(values)
        if x.dtype != np.float32:
            x = x.astype(np.float64, copy=False)
        x = np.ascontiguousarray(x)
        if x.ndim != 2 or x.shape[0] != len(ids):
            raise N.MrkError(N.ERR_INVALID_ARG, f"values of shape {x.shape} do not match {len(ids)} ids")
        p, _keep = _strs(ids)
        h = C.c_void_p()
        N.check(N.lib().mrk_index_build(ctx.handle, p, x.ctypes.data, x.dtype.itemsize, x.shape[0], x.shape[1], C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def from_encoder(cls, encoder, ids, texts, ctx: Context | None = None) -> "HipIndex":
        """BertSemanticPredictor.embed + KnnIndex.write (ml/recommend/BertSemanticRecommender.scala:61-66): the items' texts are
        embedded by a HipEncoder and the index is built from the float32 result"""
        return cls.build(ids, encoder.embed(list(texts)), ctx or encoder.ctx)

    @classmethod
    def fit_semantic(cls, encoder, ids, texts, max_tokens: int = 0) -> "HipIndex":
        """mrk_index_build_texts: BertSemanticPredictor.fit for a whole catalogue.  `texts[r]` is item r's joined text fields; the
        library cuts the catalogue into forward passes of at most `max_tokens` tokens (0: its default) and writes the pooled
        embeddings straight into the index table on the device."""
        ids, texts = list(ids), list(texts)
        if len(ids) != len(texts):
            raise N.MrkError(N.ERR_INVALID_ARG, f"{len(texts)} texts do not match {len(ids)} ids")
        pi, _ki = _strs(ids)
        pt, _kt = _strs(texts)
        h = C.c_void_p()
        N.check(N.lib().mrk_index_build_texts(encoder.ctx.handle, encoder.handle, pi, pt, len(ids), max_tokens, C.byref(h)))
        return cls(h, encoder.ctx)

    @classmethod
    def fit_similar(cls, config, users, items, ctx: Context | None = None, seed: int = 0, init=None, batches: int = 1) -> "HipIndex":
        """mrk_als_begin + add (the stream cut into `batches` calls) + fit: MFPredictor.fit with ALSRecImpl.train
        (ml/recommend/MFRecommender.scala:26-37).  `config`: ALSConfig as a dict or JSON text; `users[k]`, `items[k]`: the k-th
        (user, item) line of MFPredictor.uirt.  The item factors are computed on the device and written straight into the table."""
        from .als import AlsBuilder

        b = AlsBuilder(config, ctx)
        try:
            n = len(users)
            cuts = [n * k // batches for k in range(batches + 1)]
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                b.add(users[lo:hi], items[lo:hi])
            return b.fit(seed=seed, init=init)
        finally:
            b.close()

    def vectors(self, rows=None) -> np.ndarray:
        """mrk_index_vectors: the stored vectors of `rows` (default: all of them) as float64, len(rows) x cols"""
        info = self.info()
        r = np.arange(info["rows"], dtype=np.int64) if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        out = np.empty((len(r), info["cols"]), dtype=np.float64)
        N.check(N.lib().mrk_index_vectors(self.handle, r.ctypes.data, len(r), out.ctypes.data))
        return out

    @property
    def handle(self):
        if not self._h:
            raise N.MrkError(N.ERR_INVALID_ARG, "index is closed")
        return self._h

    def info(self) -> dict:
        rows, dev = C.c_int64(), C.c_int64()
        cols, eb = C.c_int(), C.c_int()
        N.check(N.lib().mrk_index_info(self.handle, C.byref(rows), C.byref(cols), C.byref(eb), C.byref(dev)))
        return {"rows": rows.value, "cols": cols.value, "stored_elem_bytes": eb.value, "device_bytes": dev.value}

    def ids(self, rows=None) -> list[str]:
        """the ids of `rows` (default: all of them)"""
        L = N.lib()
        rows = range(self.info()["rows"]) if rows is None else rows
        return [L.mrk_index_id(self.handle, int(r)).decode("utf-8", "surrogatepass") for r in rows]

    def row(self, item_id: str) -> int:
        return N.lib().mrk_index_row(self.handle, item_id.encode("utf-8", "surrogatepass"))

    def search(self, queries, n: int):
        """mrk_index_search: (rows, distances), each a list with one array per query (min(n, rows) entries, nearest first)"""
        q = np.ascontiguousarray(queries, dtype=np.float64)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.info()["cols"]:
            raise N.MrkError(N.ERR_INVALID_ARG, f"queries of shape {q.shape} for an index of {self.info()['cols']} columns")
        nq = q.shape[0]
        rows = np.zeros((nq, max(n, 1)), dtype=np.int32)
        dist = np.zeros((nq, max(n, 1)), dtype=np.float64)
        cnt = np.zeros(max(nq, 1), dtype=np.int32)
        N.check(N.lib().mrk_index_search(self.handle, q.ctypes.data, nq, n, rows.ctypes.data, dist.ctypes.data, cnt.ctypes.data))
        return [rows[i, :cnt[i]].copy() for i in range(nq)], [dist[i, :cnt[i]].copy() for i in range(nq)]

    def _by_items(self, fn, items, n):
        p, _keep = _strs(items)
        rows = np.zeros(max(n, 1), dtype=np.int32)
        val = np.zeros(max(n, 1), dtype=np.float64)
        cnt = C.c_int32(0)
        N.check(fn(self.handle, p, len(items), n, rows.ctypes.data, val.ctypes.data, C.byref(cnt)))
        return rows[:cnt.value].copy(), val[:cnt.value].copy()

    def lookup(self, items, n: int):
        """KnnIndexReader.lookup(items, n): (rows, distances), nearest first"""
        return self._by_items(N.lib().mrk_index_lookup, items, n)

    def recommend(self, items, count: int):
        """EmbeddingSimilarityModel.predict + Recommender.recommend: (rows, scores) of the `count` nearest items that are not in
        the request, farthest first (the reference's sortBy(-score) on distances)"""
        return self._by_items(N.lib().mrk_index_recommend, items, count)

    def close(self):
        if self._h:
            N.lib().mrk_index_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
