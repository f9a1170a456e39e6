"""Host-side mirror of the reference's LambdaMART fit, for both of its backends.

Reference interfaces (ml/rank/LambdaMARTRanker.scala:161-190, config/BoosterConfig.scala:19-28):
    LambdaMARTPredictor.makeBooster(LightGBMConfig(iterations, learningRate, ndcgCutoff, maxDepth, seed, numLeaves, sampling, debias),
                                    train, test): LightGBMBooster
`fit_lambdamart(X, labels, group_offsets, valid=(X, labels, group_offsets), **config)` is that call: the gradients, histograms,
split scans and score updates happen in libmrk_hip.so (csrc/train.hip); there is no CPU path.  The algorithm is include/mrk.h's
(DESIGN.md 19): this project's, not LightGBM's bit stream.  The forest comes back as LightGBM's text format in a HipBooster.
`backend="xgboost"` is the XGBoostConfig arm of the same call (config/BoosterConfig.scala: iterations, learningRate, ndcgCutoff, maxDepth,
seed, sampling - the ROW subsample -, debias; plus lambda, gamma, min_child_weight): a level-wise grower that bins in f32 (include/mrk.h
steps 2x, 5x, 6x, 7x) and returns XGBoost's JSON, loaded with the XGBoost backend constant.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from . import _native as N
from .booster import LIGHTGBM, XGBOOST, Context, HipBooster, default_context


def _config(config) -> bytes:
    return json.dumps(config or {}).encode()


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)


def _offsets(group_offsets):
    return np.ascontiguousarray(group_offsets, dtype=np.int64).reshape(-1)


def bin_bounds(column, **config) -> np.ndarray:
    """mrk_train_bins: the upper bounds of a column's bins but the last (host only).  backend="xgboost": step 2x's bounds - f32 values,
    widened; a cell goes left of a bound when (float) x < bound"""
    col = _f64(column)
    n = C.c_int(0)
    cfg = _config(config)
    N.check(N.lib().mrk_train_bins(cfg, col.ctypes.data, col.size, None, 0, C.byref(n)))
    out = np.zeros(n.value, dtype=np.float64)
    N.check(N.lib().mrk_train_bins(cfg, col.ctypes.data, col.size, out.ctypes.data, n.value, C.byref(n)))
    return out


def kept_categories(column, **config) -> np.ndarray:
    """mrk_train_categories: the category ids of a categorical column that get a bin of their own, ascending (host only)"""
    col = _f64(column)
    n = C.c_int(0)
    cfg = _config(config)
    N.check(N.lib().mrk_train_categories(cfg, col.ctypes.data, col.size, None, 0, C.byref(n)))
    out = np.zeros(n.value, dtype=np.int32)
    N.check(N.lib().mrk_train_categories(cfg, col.ctypes.data, col.size, out.ctypes.data, n.value, C.byref(n)))
    return out


def categorical_columns(columns) -> list:
    """the `categorical` key of a fit on mrk_values' rows: the first column of every `category` feature of
    HipRanker.values_columns() (string features with encode: index, the one-dimensional referer)"""
    return [int(first) for _, first, _, kind in columns if kind == "category"]


def lambdarank_gradients(scores, labels, group_offsets, ctx: Context | None = None, **config):
    """mrk_train_gradients: (g, h) of the lambdarank objective, one f64 per row"""
    s, y, off = _f64(scores), _f64(labels), _offsets(group_offsets)
    n_groups = len(off) - 1
    rows = int(off[-1]) if n_groups >= 1 else 0
    if s.size != rows or y.size != rows:
        raise N.MrkError(N.ERR_INVALID_ARG, f"{s.size} scores / {y.size} labels, the offsets end at {rows}")
    ctx = ctx or default_context()
    g, h = np.zeros(max(rows, 1), dtype=np.float64), np.zeros(max(rows, 1), dtype=np.float64)
    N.check(N.lib().mrk_train_gradients(ctx.handle, _config(config), s.ctypes.data, y.ctypes.data, off.ctypes.data, n_groups, g.ctypes.data, h.ctypes.data))
    return g[:rows], h[:rows]


class Trainer:
    """mrk_trainer: set(0, ...), optionally set(1, ...), fit(), then model() / history() / scores().  A set whose rows are in device
    memory - a values batch's matrix - is given in pieces instead: append_device / append_batch any number of times, then seal."""

    def __init__(self, config=None, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        N.check(N.lib().mrk_train_begin(self.ctx.handle, _config(config), C.byref(self._h)))
        self._rows = {}

    def set(self, which: int, X, labels, group_offsets):
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise N.MrkError(N.ERR_INVALID_ARG, "X is not a matrix")
        y, off = _f64(labels), _offsets(group_offsets)
        rows, cols = X.shape
        if y.size != rows:
            raise N.MrkError(N.ERR_INVALID_ARG, f"{rows} rows, {y.size} labels")
        N.check(N.lib().mrk_train_set(self._h, which, X.ctypes.data, rows, cols, y.ctypes.data, off.ctypes.data, len(off) - 1))
        self._rows[which] = rows

    def append_device(self, which: int, d_ptr: int, rows: int, cols: int):
        """mrk_train_append_device: rows x cols f64 cells, row-major, at the DEVICE address d_ptr, into the trainer's staging of set
        `which`; the work that wrote them has finished, and they may be rewritten once this returns"""
        N.check(N.lib().mrk_train_append_device(self._h, which, d_ptr, rows, cols))

    def append_batch(self, which: int, batch, first_row: int = 0, rows: int | None = None):
        """rows [first_row, first_row + rows) of a values batch's device matrix (every row by default): how a host keeps some
        click-throughs and skips others without the matrix leaving the device.  The batch must have been asked for its device matrix
        BEFORE the run that assembled the rows - load_values -> device_outputs(matrix=True) -> run(None) -, as mrk_batch_device_outputs
        says: a small values run otherwise writes its rows to the host alone."""
        if not getattr(batch, "matrix_on_device", False):
            raise N.MrkError(N.ERR_INVALID_ARG, "the batch ran before device_outputs(matrix=True) asked for its matrix: the rows may not be in device memory")
        batch.sync()
        d_matrix = batch.device_outputs(matrix=True)[2]
        rows = batch.total_items - first_row if rows is None else rows
        if first_row < 0 or rows < 1 or first_row + rows > batch.total_items:
            raise N.MrkError(N.ERR_INVALID_ARG, f"rows {first_row} ... {first_row + rows} of a batch of {batch.total_items}")
        self.append_device(which, d_matrix + first_row * batch.dim * 8, rows, batch.dim)

    def seal(self, which: int, labels, group_offsets):
        """mrk_train_seal: ends the appended set with its labels and group offsets (host arrays); the bins are found on the device"""
        y, off = _f64(labels), _offsets(group_offsets)
        rows = int(off[-1]) if len(off) else 0
        if y.size != rows:
            raise N.MrkError(N.ERR_INVALID_ARG, f"the offsets end at {rows}, {y.size} labels")
        N.check(N.lib().mrk_train_seal(self._h, which, y.ctypes.data, off.ctypes.data, len(off) - 1))
        self._rows[which] = rows

    def bounds(self, col: int) -> np.ndarray:
        """mrk_train_bounds: the trainer's bounds of a numeric column of the training set, whichever path found them"""
        n = C.c_int(0)
        N.check(N.lib().mrk_train_bounds(self._h, col, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.float64)
        N.check(N.lib().mrk_train_bounds(self._h, col, out.ctypes.data, n.value, C.byref(n)))
        return out

    def fit(self):
        N.check(N.lib().mrk_train_fit(self._h))

    def model(self) -> bytes:
        need = C.c_size_t(0)
        N.check(N.lib().mrk_train_model(self._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(max(need.value, 1))
        N.check(N.lib().mrk_train_model(self._h, buf, need.value, C.byref(need)))
        return buf.raw[:need.value]

    def history(self) -> dict:
        run, best = C.c_int(0), C.c_int(0)
        N.check(N.lib().mrk_train_history(self._h, C.byref(run), C.byref(best), None, 0))
        metric = np.zeros(max(run.value, 1), dtype=np.float64)
        N.check(N.lib().mrk_train_history(self._h, C.byref(run), C.byref(best), metric.ctypes.data, run.value))
        return {"iterations_run": run.value, "best_iteration": best.value, "metric": metric[:run.value] if 1 in self._rows else metric[:0]}

    def scores(self, which: int = 0) -> np.ndarray:
        out = np.zeros(self._rows.get(which, 0), dtype=np.float64)
        N.check(N.lib().mrk_train_scores(self._h, which, out.ctypes.data))
        return out

    def close(self):
        if self._h:
            N.lib().mrk_train_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fit_lambdamart(X, labels, group_offsets, valid=None, ctx: Context | None = None, **config):
    """-> (HipBooster, history).  valid: (X, labels, group_offsets), which turns early stopping on.  history: iterations_run,
    best_iteration, metric (the validation ndcg after every iteration), model (the text), scores / valid_scores (the trainer's own, at
    the best iteration).  A fit that ends without a tree has no forest to load: the booster is None.
    Categorical columns (set-membership splits, include/mrk.h steps 2c and 5c) are named by the config:
    fit_lambdamart(X, y, off, categorical=categorical_columns(ranker.values_columns())).
    backend="xgboost": the level-wise fit; the model is XGBoost's JSON and the booster is loaded as an XGBoost one; scores are the f32
    sums the model predicts (from its base_score 0.5), widened."""
    ctx = ctx or default_context()
    t = Trainer(config, ctx)
    try:
        t.set(0, X, labels, group_offsets)
        if valid is not None:
            t.set(1, *valid)
        t.fit()
        hist = t.history()
        hist["model"] = t.model()
        hist["scores"] = t.scores(0)
        hist["valid_scores"] = t.scores(1) if valid is not None else None
    finally:
        t.close()
    booster = HipBooster(hist["model"], XGBOOST if config.get("backend") == "xgboost" else LIGHTGBM, ctx) if hist["best_iteration"] > 0 else None
    return booster, hist
