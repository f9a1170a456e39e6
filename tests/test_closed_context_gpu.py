"""GPU: what the entries that work on a context's device say once mrk_shutdown has closed it.  A context outlives its handles, so
a builder or an index made before the shutdown can still be passed in afterwards: every such entry refuses on the host with
MRK_ERR_INVALID_ARG "context is shut down" (csrc/runtime.hpp DeviceLock) before it touches the device, and the handles still
free cleanly - the last one takes the context with it."""
import ctypes as C
import json

import numpy as np
import pytest

from metarank_amd import _native as N

pytestmark = pytest.mark.gpu


def strs(*values):
    return (C.c_char_p * len(values))(*[v.encode() for v in values])


def test_entries_refuse_a_context_that_was_shut_down():
    L = N.lib()
    ctx = C.c_void_p()
    N.check(L.mrk_init((C.c_int * 1)(0), 1, C.byref(ctx)))

    # one handle of each kind, made while the context is open
    trending = C.c_void_p()
    N.check(L.mrk_trending_begin(ctx, json.dumps({"weights": [{"interaction": "click"}]}).encode(), C.byref(trending)))
    types, type_idx, ts = strs("click"), np.zeros(3, dtype=np.int32), np.array([1000, 2000, 3000], dtype=np.int64)
    N.check(L.mrk_trending_add(trending, strs("a", "b", "a"), types, 1, type_idx.ctypes.data, ts.ctypes.data, 3))
    als = C.c_void_p()
    N.check(L.mrk_als_begin(ctx, json.dumps({"factors": 2, "iterations": 1}).encode(), C.byref(als)))
    N.check(L.mrk_als_add(als, strs("u0", "u0", "u1", "u1"), strs("i0", "i1", "i0", "i1"), 4))
    vectors = np.array([[1.0, 0.0], [0.0, 1.0]])
    index = C.c_void_p()
    N.check(L.mrk_index_build(ctx, strs("i0", "i1"), vectors.ctypes.data, 8, 2, 2, C.byref(index)))

    L.mrk_shutdown(ctx)

    scores, labels, offsets = np.array([2.0, 1.0]), np.array([1.0, 0.0]), np.array([0, 2], dtype=np.int64)
    value, fitted, factors, built = C.c_double(-7.0), C.c_void_p(), C.c_void_p(), C.c_void_p()
    refused = {
        "mrk_trending_add": lambda: L.mrk_trending_add(trending, strs("c"), types, 1, type_idx.ctypes.data, ts.ctypes.data, 1),
        "mrk_trending_fit": lambda: L.mrk_trending_fit(trending, C.byref(fitted)),
        "mrk_als_fit": lambda: L.mrk_als_fit(als, 1, None, None, None, C.byref(factors)),
        "mrk_eval_scores": lambda: L.mrk_eval_scores(ctx, 0, 10, 1, 1.0, scores.ctypes.data, labels.ctypes.data, offsets.ctypes.data, 1, C.byref(value), None),
        "mrk_index_build": lambda: L.mrk_index_build(ctx, strs("i0", "i1"), vectors.ctypes.data, 8, 2, 2, C.byref(built)),
    }
    for name, call in refused.items():
        L.mrk_model_inspect(7, None, 0, None)   # (another message in between)
        assert call() == N.ERR_INVALID_ARG, (name, L.mrk_last_error())
        assert b"context is shut down" in L.mrk_last_error(), (name, L.mrk_last_error())
    assert not fitted and not factors and not built and value.value == -7.0

    # the handles go, the last of them with the context
    L.mrk_trending_builder_free(trending)
    L.mrk_als_builder_free(als)
    L.mrk_index_free(index)
    # ... and a new context on the same device works
    again = C.c_void_p()
    N.check(L.mrk_init((C.c_int * 1)(0), 1, C.byref(again)))
    N.check(L.mrk_eval_scores(again, 0, 10, 1, 1.0, scores.ctypes.data, labels.ctypes.data, offsets.ctypes.data, 1, C.byref(value), None))
    assert value.value == 1.0
    L.mrk_shutdown(again)
