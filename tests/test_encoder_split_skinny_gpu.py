"""GPU: gemm_split_skinny_kernel (csrc/encoder_split.hip) - one request's query (<= 32 token rows) on a split-bf16 handle: one 32 x 32
block per workgroup, K over four wavefronts that continue ONE accumulator chain.  It must give a token the bits of the tile kernels
(MRK_ENCODER_SPLIT_SKINNY=0 alone; the packed ragged batch on 64 x 64 tiles), and stay within the f32 handle's bars against the fp32 graph.

K / 64 steps per wavefront: h64 1 (and the smallest hand-over); h192 3 and 5; h768 12 (two groups in registers) and 48 (groups walked
inside the turn), all three epilogues at depth.  Lengths: 1 and 31 clamp rows, 9 is a query, 32 fills the block."""
import contextlib
import os

import numpy as np
import pytest

import encoder_shapes as S
from metarank_amd import _native as N
from metarank_amd.encoder import HipEncoder
from oracle import bert
from workloads import synth

pytestmark = pytest.mark.gpu
SHAPES = [(c, n) for c in ("h64", "h192", "h768") for n in (1, 9, 31, 32)]


@contextlib.contextmanager
def _skinny(value):
    os.environ["MRK_ENCODER_SPLIT_SKINNY"] = value
    N.reload_switches()
    try:
        yield
    finally:
        del os.environ["MRK_ENCODER_SPLIT_SKINNY"]
        N.reload_switches()


def _load(case):
    tj = synth.wordpiece_tokenizer_json(vocab_size=S.VOCAB, max_length=S.MAX_POS)
    return HipEncoder(synth.bert_safetensors(S.model(case), S.CASES[case]["heads"]), tj, precision="split")


def _one(n):
    """the first n tokens of the ragged batch's longest sequence, alone"""
    ids, types, _ = S.ragged_batch()
    return ids[:1, :n], types[:1, :n], np.ones((1, n), dtype=np.int32)


@pytest.mark.parametrize("case,n", SHAPES)
def test_same_bits_as_the_tiles_alone_and_in_a_packed_batch(case, n):
    ids, types, mask = S.ragged_batch()
    mask = mask.copy()
    mask[0, n:] = 0    # the sequence as row 0 of a packed batch of 259 + n rows
    one = _one(n)
    enc = _load(case)
    try:
        with _skinny("1"):
            h1, l1 = enc.hidden_ids(*one)[0], enc.score_ids(*one)
        with _skinny("0"):
            h0, l0 = enc.hidden_ids(*one)[0], enc.score_ids(*one)
        hb, lb = enc.hidden_ids(ids, types, mask)[0, :n], enc.score_ids(ids, types, mask)[:1]
    finally:
        enc.close()
    assert np.isfinite(h1).all()
    for other, what in ((h0, "MRK_ENCODER_SPLIT_SKINNY=0"), (hb, "in the packed batch")):
        assert np.array_equal(h1.view(np.uint32), np.ascontiguousarray(other).view(np.uint32)), what
    for other, what in ((l0, "MRK_ENCODER_SPLIT_SKINNY=0"), (lb, "in the packed batch")):
        assert np.array_equal(l1.view(np.uint32), other.view(np.uint32)), f"pair logit, {what}"


@pytest.mark.parametrize("case,n", SHAPES)
def test_within_the_f32_bars_of_the_fp32_graph(case, n):
    one = _one(n)
    heads = S.CASES[case]["heads"]
    want = bert.last_hidden_state(S.model(case), *one, heads=heads, fp16=False)
    want_logit = bert.cross_logits(S.model(case), *one, heads=heads, fp16=False)
    enc = _load(case)
    try:
        with _skinny("1"):
            h, logit = enc.hidden_ids(*one), enc.score_ids(*one)
    finally:
        enc.close()
    print(f"\n{case} {n} tokens: hidden |split skinny - fp32 graph| max {float(np.abs(h - want).max()):.3e} (bound {S.ATOL_F32_HIDDEN:.1e}), "
          f"logit {float(np.abs(logit - want_logit).max()):.3e} (bound {S.ATOL_F32_LOGIT:.1e})", end="")
    np.testing.assert_allclose(h, want, rtol=0, atol=S.ATOL_F32_HIDDEN)
    np.testing.assert_allclose(logit, want_logit, rtol=0, atol=S.ATOL_F32_LOGIT)
