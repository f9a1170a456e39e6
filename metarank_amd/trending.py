"""Host-side mirror of the reference's TrendingPredictor / TrendingModel for the device fit.

Reference interfaces (ml/recommend/TrendingRecommender.scala:36-134):
    TrendingPredictor(name, TrendingConfig(weights, selector)).fit(data: Stream[TrainValues]): TrendingModel
    TrendingPredictor.load(bytes): TrendingModel
    TrendingModel.predict(RecommendRequest(count)): Response;  TrendingModel.save(): bytes
`HipTrending.fit(config, ids, types, ts)` is the drop-in for fit over the stream of ItemInteraction(item, type, ts) the
reference builds at :42 (ts = the click-through's ranking timestamp; the selector is applied before).  The aggregate over the
history happens in libmrk_hip.so (csrc/trending.hip) - there is no CPU path.  A finished model is a host object.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from . import _native as N
from .booster import Context, default_context


class HipTrending:
    def __init__(self, handle):
        self._h = handle

    @classmethod
    def fit(cls, config, ids, types, ts, ctx: Context | None = None, batches: int = 1) -> "HipTrending":
        """mrk_trending_begin + add (the stream cut into `batches` calls) + fit.  `config`: a dict or JSON text; `ids`, `types`:
        sequences of str; `ts`: milliseconds"""
        b = TrendingBuilder(config, ctx)
        try:
            n = len(ids)
            cuts = [n * k // batches for k in range(batches + 1)]
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                b.add(ids[lo:hi], types[lo:hi], ts[lo:hi])
            return b.fit()
        finally:
            b.close()

    @classmethod
    def load(cls, data: bytes) -> "HipTrending":
        buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
        h = C.c_void_p()
        N.check(N.lib().mrk_trending_load(None, buf, len(data), C.byref(h)))
        return cls(h)

    @property
    def handle(self):
        if not self._h:
            raise N.MrkError(N.ERR_INVALID_ARG, "trending model is closed")
        return self._h

    def save(self) -> bytes:
        need = C.c_size_t(0)
        st = N.lib().mrk_trending_save(self.handle, None, 0, C.byref(need))
        if st != N.ERR_INVALID_ARG or need.value == 0:
            N.check(st)
        buf = (C.c_uint8 * need.value)()
        N.check(N.lib().mrk_trending_save(self.handle, buf, need.value, C.byref(need)))
        return bytes(buf)

    def info(self) -> dict:
        items, ints, now = C.c_int64(), C.c_int64(), C.c_int64()
        N.check(N.lib().mrk_trending_info(self.handle, C.byref(items), C.byref(ints), C.byref(now)))
        return {"items": items.value, "interactions": ints.value, "now_ms": now.value}

    def items(self, ranks=None) -> list[str]:
        """the ids at `ranks` of the model (default: all of them, in model order)"""
        L = N.lib()
        ranks = range(self.info()["items"]) if ranks is None else ranks
        return [L.mrk_trending_id(self.handle, int(r)).decode("utf-8", "surrogatepass") for r in ranks]

    def predict(self, count: int):
        """TrendingModel.predict(RecommendRequest(count)): (ids, scores) of the first min(count, items) items"""
        scores = np.zeros(max(min(count, self.info()["items"]), 1), dtype=np.float64)
        n = C.c_int32(0)
        N.check(N.lib().mrk_trending_predict(self.handle, count, scores.ctypes.data, C.byref(n)))
        return self.items(range(n.value)), scores[:n.value].copy()

    def close(self):
        if self._h:
            N.lib().mrk_trending_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrendingBuilder:
    """mrk_trending_builder: add() any number of times, fit() any number of times"""

    def __init__(self, config, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        text = config if isinstance(config, (str, bytes)) else json.dumps(config)
        self._h = C.c_void_p()
        N.check(N.lib().mrk_trending_begin(self.ctx.handle, text.encode() if isinstance(text, str) else text, C.byref(self._h)))

    def add(self, ids, types, ts):
        n = len(ids)
        names = sorted(set(types))
        where = {t: i for i, t in enumerate(names)}
        idx = np.fromiter((where[t] for t in types), dtype=np.int32, count=n)
        t64 = np.ascontiguousarray(ts, dtype=np.int64)
        enc = [v.encode("utf-8", "surrogatepass") if isinstance(v, str) else v for v in ids]
        p_ids = (C.c_char_p * max(n, 1))(*enc)
        p_names = (C.c_char_p * max(len(names), 1))(*[t.encode("utf-8", "surrogatepass") for t in names])
        N.check(N.lib().mrk_trending_add(self._h, p_ids, p_names, len(names), idx.ctypes.data, t64.ctypes.data, n))

    def fit(self) -> HipTrending:
        h = C.c_void_p()
        N.check(N.lib().mrk_trending_fit(self._h, C.byref(h)))
        return HipTrending(h)

    def close(self):
        if self._h:
            N.lib().mrk_trending_builder_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
