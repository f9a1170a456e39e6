"""Host-side mirror of the reference's MFPredictor with ALSRecImpl for the device fit.

Reference interfaces (ml/recommend/MFRecommender.scala:23-63, ml/recommend/mf/ALSRecImpl.scala:18-81):
    MFPredictor(name, ALSConfig(interactions, iterations, factors, userReg, itemReg, store, selector), ALSRecImpl).fit(
        data: Stream[TrainValues]): EmbeddingSimilarityModel
`AlsBuilder(config).add(users, items)` takes the (user, item) lines of MFPredictor.uirt - the host applies the selector, the
interaction type filter and the no-user rule first - and `fit()` returns the HipIndex the reference builds from the item factors.
The iterations happen in libmrk_hip.so (csrc/als.hip); there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from . import _native as N
from .booster import Context, default_context
from .index import HipIndex, _strs


def init_matrix(seed: int, matrix: int, rows: int, cols: int) -> np.ndarray:
    """mrk_als_init_matrix: the generator's initial factors of matrix 0 (users) / 1 (items)"""
    out = np.zeros((rows, cols), dtype=np.float64)
    N.check(N.lib().mrk_als_init_matrix(seed & (2**64 - 1), matrix, rows, cols, out.ctypes.data))
    return out


class AlsBuilder:
    """mrk_als_builder: add() any number of times, fit() any number of times.  host_only: no context and no device (fit refuses)"""

    def __init__(self, config, ctx: Context | None = None, host_only: bool = False):
        text = config if isinstance(config, (str, bytes)) else json.dumps(config)
        text = text.encode() if isinstance(text, str) else text
        self._h = C.c_void_p()
        if host_only:
            self.ctx = None
            N.check(N.lib().mrk_als_begin_host(text, C.byref(self._h)))
        else:
            self.ctx = ctx or default_context()
            N.check(N.lib().mrk_als_begin(self.ctx.handle, text, C.byref(self._h)))

    def add(self, users, items):
        if len(users) != len(items):
            raise N.MrkError(N.ERR_INVALID_ARG, f"{len(users)} users do not match {len(items)} items")
        pu, _ku = _strs(users)
        pi, _ki = _strs(items)
        N.check(N.lib().mrk_als_add(self._h, pu, pi, len(users)))

    def info(self) -> dict:
        v = [C.c_int64() for _ in range(4)]
        N.check(N.lib().mrk_als_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("users", "items", "pairs", "distinct_pairs"), (x.value for x in v)))

    def config(self) -> dict:
        it, k, lu, li = C.c_int(), C.c_int(), C.c_double(), C.c_double()
        N.check(N.lib().mrk_als_config(self._h, C.byref(it), C.byref(k), C.byref(lu), C.byref(li)))
        return {"iterations": it.value, "factors": k.value, "lambda_user": lu.value, "lambda_item": li.value}

    def ids(self, matrix: int) -> list[str]:
        """the user (0) / item (1) ids in inner-index order"""
        n = self.info()["users" if matrix == 0 else "items"]
        return [N.lib().mrk_als_id(self._h, matrix, k).decode("utf-8", "surrogatepass") for k in range(n)]

    def problem(self) -> dict:
        """mrk_als_problem: R_u as CSR, R_i as CSC and the confidences"""
        i = self.info()
        out = {"user_offsets": np.zeros(i["users"] + 1, dtype=np.int32), "user_items": np.zeros(i["distinct_pairs"], dtype=np.int32),
               "item_offsets": np.zeros(i["items"] + 1, dtype=np.int32), "item_users": np.zeros(i["distinct_pairs"], dtype=np.int32),
               "confidence": np.zeros(i["items"], dtype=np.float64)}
        N.check(N.lib().mrk_als_problem(self._h, *[a.ctypes.data for a in out.values()]))
        return out

    def fit(self, seed: int = 0, init=None, user_factors: bool = False):
        """mrk_als_fit: the HipIndex of the item factors; init = (users x K, items x K) initial matrices instead of the seeded
        generator; user_factors: returns (index, final user factors)"""
        i, k = self.info(), self.config()["factors"]
        keep = [None, None]
        if init is not None:
            keep = [None if m is None else np.ascontiguousarray(m, dtype=np.float64) for m in init]
            for m, rows in zip(keep, (i["users"], i["items"])):
                if m is not None and m.shape != (rows, k):
                    raise N.MrkError(N.ERR_INVALID_ARG, f"initial factors of shape {m.shape}, expected {(rows, k)}")
        P = np.zeros((i["users"], k), dtype=np.float64) if user_factors else None
        h = C.c_void_p()
        N.check(N.lib().mrk_als_fit(self._h, seed & (2**64 - 1), *[None if m is None else m.ctypes.data for m in keep],
                                    None if P is None else P.ctypes.data, C.byref(h)))
        ix = HipIndex(h, self.ctx)
        return (ix, P) if user_factors else ix

    def close(self):
        if self._h:
            N.lib().mrk_als_builder_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
