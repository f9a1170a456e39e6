"""CPU: the ranking evaluation without a device - the restatement the GPU tests compare with (tests/eval_reference.py) against
hand-computed values, labels_from_interactions, every argument check of mrk_eval_scores / mrk_model_eval that needs no model (a
model cannot be loaded without a device: MRK_ERR_DIM_MISMATCH is reached in tests/test_eval_gpu.py), the unchanged ABI numbers,
and the host half (csrc/eval_host.cpp; tests/native/eval_host_test.cpp under ASan + UBSan)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import eval_reference as E
from metarank_amd import _native
from metarank_amd.eval import labels_from_interactions, noop_array

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LABELS = [3, 2, 3, 0, 1, 2]
IN_ORDER = [6.0, 5.0, 4.0, 3.0, 2.0, 1.0]     # scores that keep the given order


def test_host_logic_native_driver(tmp_path):
    exe = str(tmp_path / "eval_host_test")
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(REPO, "tests", "native", "eval_host_test.cpp"), os.path.join(csrc, "eval_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ALL OK" in out.stdout


def test_known_answer_linear_gain():
    """the textbook example: DCG 6.861, IDCG 7.141, NDCG 0.961"""
    g = [float(y) for y in LABELS]
    assert round(E._dcg(g, 6), 3) == 6.861
    assert round(E._dcg(sorted(g, reverse=True), 6), 3) == 7.141
    assert round(E.ndcg(IN_ORDER, LABELS, 0, relpow=False), 3) == 0.961
    assert E.ndcg(None, LABELS, 0, relpow=False, pi=list(range(6))) == E.ndcg(IN_ORDER, LABELS, 0, relpow=False)


def test_hand_cases_ndcg():
    # gains 2^y - 1 = [7, 3, 7, 0, 1, 3]: 7 + 3/lg3 + 7/2 + 0 + 1/lg6 + 3/lg7 = 13.848; ideal [7, 7, 3, 3, 1, 0]: 14.595
    lg = [math.log2(i + 2) for i in range(6)]
    dcg = 7 + 3 / lg[1] + 7 / 2 + 0 + 1 / lg[4] + 3 / lg[5]
    idcg = 7 + 7 / lg[1] + 3 / 2 + 3 / lg[3] + 1 / lg[4] + 0
    assert abs(dcg - 13.848) < 1e-3 and abs(idcg - 14.595) < 1e-3
    assert abs(E.ndcg(IN_ORDER, LABELS, 0, relpow=True) - dcg / idcg) < 1e-15
    assert round(E.ndcg(IN_ORDER, LABELS, 0, relpow=True), 3) == 0.949
    assert E.ndcg(IN_ORDER, LABELS, 1, relpow=False) == 1.0                      # 3 / 3
    assert round(E.ndcg(IN_ORDER, LABELS, 3, relpow=False), 3) == 0.978          # (3 + 2/lg3 + 3/2) / (3 + 3/lg3 + 2/2) = 5.762 / 5.893
    assert E.ndcg(IN_ORDER, LABELS, 7, relpow=False) == E.ndcg(IN_ORDER, LABELS, 0, relpow=False) == E.ndcg(IN_ORDER, LABELS, 6, relpow=False)
    # the reverse order is worse, the ideal order is 1
    assert E.ndcg(IN_ORDER[::-1], LABELS, 0, relpow=False) < 0.961
    assert E.ndcg([float(y) for y in LABELS], LABELS, 0, relpow=True) == 1.0
    # no label at all: nolabels, whatever it is
    assert E.ndcg(IN_ORDER, [0] * 6, 10) == 1.0 and E.ndcg(IN_ORDER, [0] * 6, 10, nolabels=0.25) == 0.25
    assert E.ndcg(IN_ORDER, [0.0, -0.0, 0.0, 0.0, 0.0, 0.0], 10, relpow=False, nolabels=0.5) == 0.5


def test_hand_cases_map_and_mrr():
    rel = [1, 0, 1, 0, 0, 1]
    assert E.average_precision(IN_ORDER, rel, 0) == (1.0 + 2.0 / 3.0 + 3.0 / 6.0) / 3.0      # 0.7222
    assert round(E.average_precision(IN_ORDER, rel, 0), 4) == 0.7222
    assert E.average_precision(IN_ORDER, rel, 3) == (1.0 + 2.0 / 3.0) / 3.0                  # / min(R = 3, k = 3)
    assert E.average_precision(IN_ORDER, rel, 2) == 1.0 / 2.0                                # / min(3, 2)
    assert E.average_precision(IN_ORDER, [0, 0, 0, 0, 0, 5], 3) == 0.0                       # relevant, but behind the cutoff
    assert E.average_precision(IN_ORDER, [0] * 6, 0) == 0.0
    assert E.average_precision(IN_ORDER, [0.5] * 6, 0) == 1.0                                # fractional labels are relevant
    assert E.reciprocal_rank([4.0, 3.0, 2.0, 1.0], [0, 0, 1, 0]) == 1.0 / 3.0
    assert E.reciprocal_rank([1.0, 2.0, 3.0, 4.0], [0, 0, 1, 0]) == 1.0 / 2.0
    assert E.reciprocal_rank([4.0, 3.0, 2.0, 1.0], [0, 0, -1, 0]) == 0.0
    assert E.group_value(E.MRR, 1, [4.0, 3.0, 2.0, 1.0], [0, 0, 1, 0]) == 1.0 / 3.0          # MRR ignores the cutoff


def test_order_is_the_rank_order():
    nan, inf = float("nan"), float("inf")
    assert E.order([1.0, nan, 3.0, 3.0, -inf, inf, -0.0, 0.0]) == [5, 2, 3, 0, 7, 6, 4, 1]   # NaN last, +0.0 before -0.0, ties in place
    off = [0, 4, 5, 8]
    assert np.array_equal(E.noop_array(off), noop_array(off))
    assert list(E.noop_array(off)) == [1.0, 0.75, 0.5, 0.25, 1.0, 1.0, 2.0 / 3.0, 1.0 / 3.0]
    assert E.orders(E.noop_array(off), off) == [[0, 1, 2, 3], [0], [0, 1, 2]]               # strictly decreasing: the identity
    assert E.mean([0.1, 0.2, 0.3]) == (0.1 + 0.2 + 0.3) / 3.0


def test_labels_from_interactions():
    w = {"click": 1.0, "purchase": 3.0}
    items = ["a", "b", "c", "d", "e"]
    ints = [("b", "click"), ("b", "purchase"),            # the first interaction naming the item decides
            ("c", "purchase", 0.5),                       # rel beats the weight
            {"item": "d", "type": "view"},                # an unknown type: 0
            {"item": "e", "type": "view", "rel": 2}, ("zz", "click")]
    assert list(labels_from_interactions(items, ints, w)) == [0.0, 1.0, 0.5, 0.0, 2.0]
    assert list(labels_from_interactions(items, [], w)) == [0.0] * 5
    assert list(labels_from_interactions(["b"], [("b", "purchase"), ("b", "click", 9)], w)) == [3.0]


def test_argument_checks_come_before_any_device_work():
    L = _native.lib()
    INVALID = _native.ERR_INVALID_ARG
    s = np.array([3.0, 2.0, 1.0, 5.0, 4.0])
    y = np.array([0.0, 1.0, 2.0, 0.0, 1.0])
    off = np.array([0, 3, 5], dtype=np.int64)
    val = C.c_double(-7.0)

    def p(a):
        return None if a is None else a.ctypes.data

    def scores(metric=0, cutoff=10, flags=1, s=s, y=y, off=off, n=2, out=val):
        st = L.mrk_eval_scores(None, metric, cutoff, flags, 1.0, p(s), p(y), p(off), n, None if out is None else C.byref(out), None)
        return st, L.mrk_last_error()

    def model(metric=0, cutoff=10, flags=1, s=s, cols=1, y=y, off=off, n=2, out=np.zeros(3), metrics="one", cutoffs="one", nm=1):
        ms = np.array([metric], dtype=np.int32) if isinstance(metrics, str) else metrics
        ks = np.array([cutoff], dtype=np.int32) if isinstance(cutoffs, str) else cutoffs
        st = L.mrk_model_eval(None, p(ms), p(ks), nm, flags, 1.0, p(s), cols, p(y), p(off), n, None, p(out), None)
        return st, L.mrk_last_error()

    # everything in order but the context / the model: that is the last thing asked for
    assert scores() == (INVALID, b"null context")
    assert model() == (INVALID, b"null model")
    refused = [(dict(metric=3), b"unknown metric 3"), (dict(metric=-1), b"unknown metric -1"), (dict(cutoff=-1), b"negative cutoff"),
               (dict(flags=2), b"unknown flags"), (dict(n=0), b"no groups"), (dict(n=-5), b"no groups"), (dict(off=None), b"null group offsets"),
               (dict(y=None), b"null labels"), (dict(out=None), b"null"), (dict(s=None), b"null"),
               (dict(off=np.array([1, 3, 5], dtype=np.int64)), b"do not start at 0"),
               (dict(off=np.array([0, 3, 3], dtype=np.int64)), b"empty"),
               (dict(off=np.array([0, 3, 2], dtype=np.int64)), b"decrease"),
               (dict(y=np.array([0.0, np.nan, 2.0, 0.0, 1.0])), b"label 1 is not finite"),
               (dict(y=np.array([0.0, 1.0, 2.0, 0.0, np.inf])), b"label 4 is not finite")]
    for call in (scores, model):
        for bad, what in refused:
            st, msg = call(**bad)
            assert st == INVALID and what in msg, (call.__name__, bad, st, msg)
    assert model(cols=-1)[0] == INVALID
    assert model(metrics=None)[0] == INVALID and model(cutoffs=None)[0] == INVALID
    assert model(nm=0) == (INVALID, b"eval: no metric asked for")
    two = np.array([0, 7], dtype=np.int32)
    assert model(metrics=two, cutoffs=two, nm=2) == (INVALID, b"eval: unknown metric 7")
    assert scores(off=np.array([0, 2**30 + 1], dtype=np.int64), n=1)[0] == _native.ERR_UNSUPPORTED   # (judged from the offsets alone)
    assert val.value == -7.0
    assert L.mrk_abi_version() == 9 and L.mrk_abi_layout(None, 0) == 33   # new symbols only
