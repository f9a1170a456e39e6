"""GPU: step 2d of the LambdaMART fit (include/mrk.h, csrc/train_bins.hip) - the trainer's matrix appended from device memory, its bins
found on the device.  The yardsticks are what exists without it: mrk_train_bins (train.bin_bounds) for the bounds, and the host path
mrk_train_set -> mrk_train_model / mrk_train_scores / mrk_train_history for everything downstream.  Every comparison is by bit
pattern or bytes."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import metarank_amd as M
from backends import HipBackend
from metarank_amd import _native as N
from metarank_amd.train import Trainer, bin_bounds
from workloads import ranklens, synth

pytestmark = pytest.mark.gpu

_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipFree.argtypes = [C.c_void_p]
    return _hip


class DeviceMatrix:
    """a row-major f64 matrix in device memory, through the HIP runtime"""

    def __init__(self, X):
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.rows, self.cols = self.X.shape
        self.p = C.c_void_p()
        assert hip().hipMalloc(C.byref(self.p), max(self.X.nbytes, 8)) == 0
        assert hip().hipMemcpy(self.p, self.X.ctypes.data, self.X.nbytes, 1) == 0

    def at(self, row):
        return self.p.value + row * self.cols * 8

    def free(self):
        if self.p:
            hip().hipFree(self.p)
            self.p = C.c_void_p()


def give(t, which, X, y, off, device, pieces=None):
    """the set through mrk_train_set, or appended from device memory in `pieces` (row counts; one piece by default) and sealed"""
    if not device:
        t.set(which, X, y, off)
        return
    d = DeviceMatrix(X)
    try:
        row = 0
        for n in pieces or [d.rows]:
            t.append_device(which, d.at(row), n, d.cols)
            row += n
        assert row == d.rows
        t.seal(which, y, off)
    finally:
        d.free()


def one_group_per(n, size=1000):
    return np.array(list(range(0, n, size)) + [n], dtype=np.int64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def fitted(t):
    t.fit()
    h = t.history()
    return t.model(), bits(t.scores(0)), (bits(t.scores(1)) if 1 in t._rows else None), h["iterations_run"], h["best_iteration"], bits(h["metric"])


# ---- bounds ------------------------------------------------------------------------------------------------------------------------

ROW_COUNTS = [1, 2, 255, 256, 257, 4095, 4096, 4097, 40_000]   # one workgroup orders up to 4 096 cells, the sample sort more (40 000: 64 buckets)


def bound_columns(n, xgb):
    """name -> column of n cells: the plain shapes and the adversarial ones of tests/native/train_cuts_test.cpp"""
    rng = np.random.default_rng(n)
    k = np.arange(n, dtype=np.float64)
    big = 3.3e38 - (k % 400) * 1e32 if xgb else 1.7e308 - (k % 400) * 4e292    # (1.7e308 is no f32: step 2x would refuse it)
    cols = {
        "all NaN": np.full(n, np.nan),
        "constant": np.full(n, 2.5),
        "boolean": (rng.random(n) < 0.3).astype(np.float64),
        "ten values": rng.integers(0, 10, n).astype(np.float64),
        "distinct": rng.permutation(n) * 0.25 - 7.0,
        "half NaN": np.where(np.arange(n) % 2 == 0, np.nan, rng.normal(size=n)),
        "a run across quantile positions": rng.permutation(np.where(np.arange(n) % 3 == 0, k, 150.0)),
        "a last run to the end": rng.permutation(np.where(np.arange(n) < n // 10, k, 1e6)),
        "one ulp apart": rng.permutation(1.0 + (k % 600) * 2.0 ** -52),
        "overflowing sums": rng.permutation(np.where(np.arange(n) % 2 == 0, big, -big)),
        "zeros": rng.choice([-0.0, 0.0, 1.0, -1.0], n),
        "f32 neighbours": 1.0 + rng.integers(0, 4096, n) * 2.0 ** -30,    # 128 f64 values share an f32
    }
    return cols


@pytest.mark.parametrize("backend", ["lightgbm", "xgboost"])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_bounds_are_the_host_bin_finders(ctx, n, backend):
    xgb = backend == "xgboost"
    cols = bound_columns(n, xgb)
    names = list(cols)
    X = np.stack([cols[c] for c in names], axis=1)
    for max_bin in (4, 16):
        cfg = {"backend": backend, "max_bin": max_bin} if xgb else {"max_bin": max_bin}
        want = {c: bin_bounds(cols[c], **cfg) for c in names}
        if n >= 4095:   # the inputs take the branches they are here for (judged on the CPU)
            distinct = {c: len(np.unique(cols[c][~np.isnan(cols[c])] if not xgb else cols[c][~np.isnan(cols[c])].astype(np.float32))) for c in names}
            assert distinct["all NaN"] == 0 and len(want["all NaN"]) == 0 and distinct["constant"] == 1 and len(want["constant"]) == 0
            assert distinct["boolean"] == 2 <= max_bin - 1 and len(want["boolean"]) == 1                   # every change is a cut
            assert distinct["distinct"] > max_bin - 1 and len(want["distinct"]) == max_bin - 2             # the quantile rule, every cut kept
            for c in ("a run across quantile positions", "a last run to the end"):                         # the quantile rule, cuts dropped / none left
                assert distinct[c] > max_bin - 1 and len(want[c]) < max_bin - 2, (c, len(want[c]))
            assert len(want["a run across quantile positions"]) >= 1
            if not xgb:
                assert len(want["one ulp apart"]) >= 2 and set(want["one ulp apart"]) <= set(cols["one ulp apart"])   # every bound fell back to a
                over = want["overflowing sums"]                # a + b overflowed: the bound is a itself, or -inf between two negative cells
                assert len(over) >= 2 and all(np.isneginf(b) or b in set(cols["overflowing sums"]) for b in over)
        t = Trainer(cfg, ctx)
        try:
            give(t, 0, X, np.zeros(n), one_group_per(n), device=True)
            for j, c in enumerate(names):
                got = t.bounds(j)
                assert bits(got) == bits(want[c]), (n, backend, max_bin, c, len(got), len(want[c]))
        finally:
            t.close()


def test_bounds_of_the_host_path_and_the_refusals_of_mrk_train_bounds(ctx):
    X, y, off = synth.synthetic_ranking_rows(20, 10, 30, 8, seed=3)
    X[:, 7] = np.clip(np.rint(X[:, 7] * 3.0 + 5.0), 0, 12)
    t = Trainer({"max_bin": 16, "categorical": [7]}, ctx)
    try:
        with pytest.raises(N.MrkError) as e:
            t.bounds(0)                                        # before any set
        assert e.value.status == N.ERR_INVALID_ARG
        t.set(0, X, y, off)
        for c in range(7):
            assert bits(t.bounds(c)) == bits(bin_bounds(X[:, c], max_bin=16))
        for c in (7, 8, -1):                                   # categorical, outside the matrix
            with pytest.raises(N.MrkError) as e:
                t.bounds(c)
            assert e.value.status == N.ERR_INVALID_ARG
    finally:
        t.close()


# ---- pieces, end to end -----------------------------------------------------------------------------------------------------------------

def rows_for_a_fit(categorical=False):
    X, y, off = synth.synthetic_ranking_rows(120, 10, 100, 24, seed=5)
    Xv, yv, offv = synth.synthetic_ranking_rows(30, 10, 100, 24, seed=6)
    if categorical:
        for mat in (X, Xv):
            mat[:, 22:] = np.clip(np.rint((mat[:, 22:] + 3.0) * (49.0 / 6.0)), 0.0, 49.0)
        y, yv = X[:, 22] % 5.0, Xv[:, 22] % 5.0   # labels only a set of categories explains
        Xv[::7, 23] = 77.0       # a category the training set never saw
        X[::11, 22] = -3.0       # no category
        X[::13, 22] = np.nan
    return (X, y, off), (Xv, yv, offv)


CONFIGS = {
    "lightgbm": {"iterations": 4, "numLeaves": 8, "max_bin": 32, "early_stopping": 4},
    "categorical": {"iterations": 4, "numLeaves": 8, "max_bin": 16, "early_stopping": 4, "categorical": [22, 23], "min_data_per_group": 10, "cat_smooth": 1.0},
    "xgboost": {"backend": "xgboost", "iterations": 4, "maxDepth": 4, "max_bin": 32, "early_stopping": 4},
}


def test_pieces_give_the_bounds_and_the_model_of_one_piece(ctx):
    (X, y, off), _ = rows_for_a_fit()
    rows = X.shape[0]
    assert rows > 4097 + 1
    results = []
    for pieces in (None, [1, 4096, rows - 4097]):
        t = Trainer(CONFIGS["lightgbm"], ctx)
        try:
            give(t, 0, X, y, off, device=True, pieces=pieces)
            b = [bits(t.bounds(c)) for c in range(X.shape[1])]
            results.append((b, fitted(t)))
        finally:
            t.close()
    assert results[0] == results[1]
    assert results[0][0] == [bits(bin_bounds(X[:, c], max_bin=32)) for c in range(X.shape[1])]
    assert results[0][1][4] >= 1   # a forest, not an empty model


@pytest.mark.parametrize("name", list(CONFIGS))
def test_device_sets_fit_the_model_of_host_sets(ctx, name):
    train, valid = rows_for_a_fit(categorical=name == "categorical")
    got = {}
    for dev_train, dev_valid in ((False, False), (True, True), (False, True), (True, False)):
        t = Trainer(CONFIGS[name], ctx)
        try:
            give(t, 0, *train, device=dev_train, pieces=[1000, train[0].shape[0] - 1000] if dev_train else None)
            give(t, 1, *valid, device=dev_valid)
            got[(dev_train, dev_valid)] = fitted(t)
        finally:
            t.close()
    want = got[(False, False)]
    assert want[4] >= 1 and len(want[5]) == want[3]
    if name == "categorical":
        assert re.search(rb"num_cat=[1-9]", want[0])   # the fit went through a categorical column's bins
    for k, v in got.items():
        assert v == want, k


@contextlib.contextmanager
def interpreting_kernels():
    """MRK_RANK_JIT=0 for the block: the values rows come from the interpreting kernels, no specialised kernel is compiled for them"""
    saved = os.environ.get("MRK_RANK_JIT")
    os.environ["MRK_RANK_JIT"] = "0"
    M.reload_switches()
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop("MRK_RANK_JIT", None)
        else:
            os.environ["MRK_RANK_JIT"] = saved
        M.reload_switches()


def test_rows_of_a_values_batch_by_range(ctx):
    with interpreting_kernels():
        rows_of_a_values_batch_by_range(ctx)


def rows_of_a_values_batch_by_range(ctx):
    cfg = ranklens.ranklens_config()
    be = HipBackend(cfg, "xgboost", ctx)
    try:
        ranklens.load_state(be, ranklens.generate_state(300, 40))
        reqs = ranklens.generate_requests(3, 40, 300, 40, seed=5)
        batch = be.ranker.new_batch()
        try:
            batch.load_values(reqs)
            batch.run(None)
            t = Trainer({}, ctx)
            with pytest.raises(N.MrkError):                                 # the matrix was not asked for before the run
                t.append_batch(0, batch)
            t.close()
            batch.device_outputs(matrix=True)
            batch.run(None)
            off = batch.offsets
            keep = (0, 2)                                                   # the middle click-through had no interaction: skipped
            fit_cfg = {"iterations": 3, "numLeaves": 4, "min_data_in_leaf": 1, "max_bin": 16, "min_sum_hessian": 0.0}
            rng = np.random.default_rng(9)
            y = np.concatenate([rng.integers(0, 3, int(off[g + 1] - off[g])).astype(np.float64) for g in keep])
            goff = np.concatenate([[0], np.cumsum([int(off[g + 1] - off[g]) for g in keep])]).astype(np.int64)
            t = Trainer(fit_cfg, ctx)
            try:
                for g in keep:
                    t.append_batch(0, batch, first_row=int(off[g]), rows=int(off[g + 1] - off[g]))
                t.seal(0, y, goff)
                dev_bounds = [bits(t.bounds(c)) for c in range(batch.dim)]
                dev = fitted(t)
            finally:
                t.close()
            mat = batch.fetch(matrix=True)[2]
            X = np.concatenate([mat[int(off[g]):int(off[g + 1])] for g in keep])
            assert X.shape == (int(goff[-1]), batch.dim) and len({tuple(r) for r in X.tolist()}) > 1
            t = Trainer(fit_cfg, ctx)
            try:
                t.set(0, X, y, goff)
                host_bounds = [bits(t.bounds(c)) for c in range(batch.dim)]
                host = fitted(t)
            finally:
                t.close()
            assert dev_bounds == host_bounds and dev == host
            # every row, the default range
            t = Trainer(fit_cfg, ctx)
            try:
                t.append_batch(0, batch)
                t.seal(0, np.zeros(batch.total_items), off)
                assert [bits(t.bounds(c)) for c in range(batch.dim)] == [bits(bin_bounds(mat[:, c], max_bin=16)) for c in range(batch.dim)]
            finally:
                t.close()
        finally:
            batch.close()
    finally:
        be.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def named_cell(message):
    m = re.search(r"column (\d+), row (\d+)", message)
    assert m, message
    return int(m.group(2)), int(m.group(1))


def small_sets():
    X, y, off = synth.synthetic_ranking_rows(12, 10, 40, 8, seed=21)
    Xv, yv, offv = synth.synthetic_ranking_rows(5, 10, 40, 8, seed=22)
    return (X, y, off), (Xv, yv, offv)


REFUSAL_CFG = {"iterations": 2, "numLeaves": 4, "max_bin": 16, "min_data_in_leaf": 1}


def host_status(cfg, ctx, train, valid=None):
    t = Trainer(cfg, ctx)
    try:
        t.set(0, *train)
        if valid is not None:
            t.set(1, *valid)
    except N.MrkError as e:
        return e.status
    finally:
        t.close()
    return 0


def good_fit(t, cfg, ctx, train, valid):
    """after a refusal the trainer still takes a correct set from the device and fits the host path's model"""
    give(t, 0, *train, device=True)
    give(t, 1, *valid, device=True)
    got = fitted(t)
    h = Trainer(cfg, ctx)
    try:
        h.set(0, *train)
        h.set(1, *valid)
        assert got == fitted(h)
    finally:
        h.close()


@pytest.mark.parametrize("case", ["infinite, training", "infinite, validation", "1e300 under xgboost", "category 32765"])
def test_refused_cells_keep_the_host_paths_status_and_name_a_cell_that_holds_one(ctx, case):
    train, valid = small_sets()
    cfg = dict(REFUSAL_CFG)
    bad_train, bad_valid = [m.copy() for m in (train[0], valid[0])]
    which = 0
    if case == "infinite, training":
        bad_train[17, 2], bad_train[40, 3] = np.inf, -np.inf
        status, holds = N.ERR_INVALID_ARG, np.isinf
    elif case == "infinite, validation":
        which = 1
        bad_valid[9, 1], bad_valid[30, 0] = -np.inf, np.inf
        status, holds = N.ERR_INVALID_ARG, np.isinf
    elif case == "1e300 under xgboost":
        cfg = {"backend": "xgboost", "iterations": 2, "maxDepth": 3, "max_bin": 16}
        bad_train[5, 1], bad_train[60, 0] = 1e300, -1e300
        status, holds = N.ERR_INVALID_ARG, lambda v: abs(v) == 1e300
    else:
        cfg["categorical"] = [3]
        for m in (train[0], valid[0], bad_train, bad_valid):
            m[:, 3] = np.clip(np.rint(m[:, 3] * 2.0 + 4.0), 0, 9)
        bad_train[9, 3], bad_train[33, 3] = 32765.0, 40000.0
        bad_train[10, 0] = 50000.0                             # a numeric column: no category
        status, holds = N.ERR_UNSUPPORTED, lambda v: v >= 32765.0
    assert host_status(cfg, ctx, (bad_train, train[1], train[2]), (bad_valid, valid[1], valid[2])) == status
    t = Trainer(cfg, ctx)
    try:
        if which == 1:
            give(t, 0, *train, device=True)
        bad = bad_train if which == 0 else bad_valid
        with pytest.raises(N.MrkError) as e:
            give(t, which, bad, *(train if which == 0 else valid)[1:], device=True, pieces=[7, bad.shape[0] - 7])
        assert e.value.status == status
        row, col = named_cell(e.value.message)
        assert holds(bad[row, col]), (e.value.message, bad[row, col])
        if case == "category 32765":
            assert col == 3 and ("32765" in e.value.message or "40000" in e.value.message)
        good_fit(t, cfg, ctx, train, valid)
    finally:
        t.close()


def test_state_refusals(ctx):
    train, valid = small_sets()
    X, y, off = train
    t = Trainer(REFUSAL_CFG, ctx)
    d, dv = DeviceMatrix(X), DeviceMatrix(valid[0])
    try:
        # the validation set before the training set
        t.append_device(1, dv.at(0), dv.rows, dv.cols)
        with pytest.raises(N.MrkError) as e:
            t.seal(1, valid[1], valid[2])
        assert e.value.status == N.ERR_INVALID_ARG and "after the training set" in e.value.message
        # nothing appended
        with pytest.raises(N.MrkError) as e:
            t.seal(0, y, off)
        assert e.value.status == N.ERR_INVALID_ARG
        # offsets that do not end at the staged rows
        t.append_device(0, d.at(0), d.rows - 1, d.cols)
        with pytest.raises(N.MrkError) as e:
            t.seal(0, y, off)
        assert e.value.status == N.ERR_INVALID_ARG and "do not end" in e.value.message
        # cols changing between appends; null pointer; rows < 1
        t.append_device(0, d.at(0), 10, d.cols)
        for args in ((d.at(0), 5, d.cols - 1), (None, 5, d.cols), (d.at(0), 0, d.cols), (d.at(0), 5, 0)):
            with pytest.raises(N.MrkError) as e:
                t.append_device(0, *args)
            assert e.value.status == N.ERR_INVALID_ARG, args
        # the pieces before the refused ones are still there: the rest of the rows, and the set is whole
        t.append_device(0, d.at(10), d.rows - 10, d.cols)
        t.seal(0, y, off)
        # mrk_train_set on a set with staged rows drops them
        t.append_device(1, dv.at(0), 3, dv.cols)
        t.set(1, *valid)
        with pytest.raises(N.MrkError) as e:
            t.seal(1, valid[1], valid[2])
        assert e.value.status == N.ERR_INVALID_ARG
        got = fitted(t)
        h = Trainer(REFUSAL_CFG, ctx)
        try:
            h.set(0, *train)
            h.set(1, *valid)
            assert got == fitted(h)
        finally:
            h.close()
        # a fitted trainer takes nothing more
        with pytest.raises(N.MrkError) as e:
            t.append_device(0, d.at(0), 5, d.cols)
        assert e.value.status == N.ERR_INVALID_ARG
    finally:
        t.close()
        d.free()
        dv.free()
