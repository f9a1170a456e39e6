"""GPU: the wavefront-per-request ordering (csrc/rank.hip sort_wave_kernel: batches whose largest request has <= 128 candidates).
One batch of 9 requests of 1, 2, 63, 64, 65, 100, 127, 128, 100 candidates (nine is no multiple of the four requests a
workgroup orders: the last workgroup is partly empty) and one of 129 / 100 / 256 (the old kernel), ranked through prepare / run / fetch
and then re-ordered (mrk_batch_sort) over constructed scores - ties, runs of ties across candidates 63 / 64, NaNs of both signs, +-0,
+-inf - bit for bit against the oracle's sort_order and against the parent rule (stable order of (sort_key, index))."""
import ctypes as C

import numpy as np
import pytest

from backends import HipBackend
from oracle.assembly import sort_order
from workloads import ranklens
import eval_reference

WAVE, COUNTING = 2, 1   # mrk_debug_batch_order's ordering launch
NAN_N = np.frombuffer(np.uint64(0xfff8000000000000).tobytes(), dtype=np.float64)[0]
NAN_PAYLOAD = np.frombuffer(np.uint64(0x7ff0000000000123).tobytes(), dtype=np.float64)[0]


def same(a, b):
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def constructed_scores(n, seed):
    """ties, a run of ties across candidates 63 / 64, NaNs of both signs, +-0, +-inf, a few ordinary values"""
    rng = np.random.Generator(np.random.PCG64(seed))
    special = np.array([np.nan, NAN_N, NAN_PAYLOAD, 0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 2.5, 2.5, 5e-324])
    v = special[rng.integers(0, len(special), n)]
    v[60:70] = 2.5   # (a no-op for n <= 60)
    return v


def order_batch(hip, hiprt, sizes, form):
    reqs = [{"id": f"r{k}", "timestamp": ranklens.TS, "user": None, "session": None, "fields": [], "items": [{"id": f"x{k}_{i}"} for i in range(n)]}
            for k, n in enumerate(sizes)]
    batch = hip.ranker.prepare("xgboost", reqs)
    try:
        batch.run(None)   # NoopRanker: every score 0.0 - all ties, the order is the request's own
        scores, order, _ = batch.fetch()
        assert batch.order_info()["sort"] == form, batch.order_info()
        for r, n in enumerate(sizes):
            lo, hi = batch.offsets[r], batch.offsets[r + 1]
            assert hi - lo == n and not scores[lo:hi].any() and order[lo:hi].tolist() == list(range(n)), r
        for seed in (1, 2):
            want = np.concatenate([constructed_scores(n, 10 * seed + r) for r, n in enumerate(sizes)])
            batch.sync()
            assert hiprt.hipMemcpy(batch.device_outputs()[0], want.ctypes.data, want.nbytes, 1) == 0
            batch.sort()
            scores, order, _ = batch.fetch()
            assert batch.order_info()["sort"] == form
            assert same(scores, want)
            for r, n in enumerate(sizes):
                lo, hi = batch.offsets[r], batch.offsets[r + 1]
                assert order[lo:hi].tolist() == sort_order(want[lo:hi]).tolist(), (seed, r, n)
                assert order[lo:hi].tolist() == sorted(range(n), key=lambda i: (eval_reference.sort_key(float(want[lo + i])), i)), (seed, r, n)
    finally:
        batch.close()


@pytest.mark.gpu
def test_small_requests_take_the_wavefront_kernel_and_larger_batches_the_old_one():
    hiprt = C.CDLL("libamdhip64.so")
    hiprt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip = HipBackend(ranklens.ranklens_config(), "xgboost")
    try:
        order_batch(hip, hiprt, [1, 2, 63, 64, 65, 100, 127, 128, 100], WAVE)
        order_batch(hip, hiprt, [129, 100, 256], COUNTING)
    finally:
        hip.close()
