"""GPU: attention_split_kernel (csrc/encoder_split.hip) - a split-bf16 handle's attention under MRK_ENCODER_SPLIT_ATTENTION=1: Q K^T and
P V as split products on the bf16 instruction, 32 queries x 32 keys a block, softmax in f32.  Held to the f32 handle's bars against the
fp32 graph, to bits that depend on a sequence's own tokens only, and to the switch: 0 and unset are the kernel of before.

h64: one head of size 64 (three wavefronts leave); h192: six heads of size 32 (a group of four and one of two); h768: twelve of size 64.
The ragged lengths lie on both sides of every 16- and 32-row / key boundary; the holes batch has a dead first block, a dead middle
block and a sequence whose only live key is its last."""
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


@contextlib.contextmanager
def _env(name, value):
    os.environ[name] = value
    N.reload_switches()
    try:
        yield
    finally:
        del os.environ[name]
        N.reload_switches()


def _load(case):
    tj = synth.wordpiece_tokenizer_json(vocab_size=S.VOCAB, max_length=S.MAX_POS)
    return HipEncoder(synth.bert_safetensors(S.model(case), S.CASES[case]["heads"]), tj, precision="split")


@pytest.mark.parametrize("case,batch", [(c, b) for c in ("h64", "h192", "h768") for b in S.BATCHES])
def test_within_the_f32_bars_of_the_fp32_graph(case, batch):
    ids, types, mask = S.BATCHES[batch]()
    live = mask.astype(bool)
    want = S.oracle_hidden(case, "f32", batch)
    with _env("MRK_ENCODER_SPLIT_ATTENTION", "1"):
        enc = _load(case)
        try:
            h = enc.hidden_ids(ids, types, mask)
            logits = enc.score_ids(ids, types, mask) if batch == "ragged" else None
        finally:
            enc.close()
    print(f"\n{case} {batch}: hidden |split attention - fp32 graph| max {float(np.abs(h - want)[live].max()):.3e} (bound {S.atol(case, 'f32'):.1e})", end="")
    assert np.isfinite(h[live]).all()
    np.testing.assert_allclose(h[live], want[live], rtol=0, atol=S.atol(case, "f32"))
    if logits is not None:
        want_logits = bert.cross_logits(S.model(case), ids, types, mask, heads=S.CASES[case]["heads"], fp16=False)
        print(f", logits {float(np.abs(logits - want_logits).max()):.3e} (bound {S.ATOL_F32_LOGIT:.1e})", end="")
        np.testing.assert_allclose(logits, want_logits, rtol=0, atol=S.ATOL_F32_LOGIT)


@pytest.mark.parametrize("case", ["h192", "h768"])
def test_a_sequence_has_the_same_bits_alone_padded_and_packed(case):
    ids, types, mask = S.ragged_batch()
    ones = lambda n: np.ones((1, n), dtype=np.int32)
    with _env("MRK_ENCODER_SPLIT_ATTENTION", "1"):
        enc = _load(case)
        try:
            packed = enc.embed_ids(ids, types, mask)
            with _env("MRK_ENCODER_PACKED", "0"):
                padded = enc.embed_ids(ids, types, mask)
            alone = np.concatenate([enc.embed_ids(ids[b:b + 1, :n], types[b:b + 1, :n], ones(n)) for b, n in enumerate(S.RAGGED_LENS)])
            hidden = enc.hidden_ids(ids, types, mask)
            hidden_alone = [enc.hidden_ids(ids[b:b + 1, :n], types[b:b + 1, :n], ones(n))[0] for b, n in enumerate(S.RAGGED_LENS)]
        finally:
            enc.close()
    assert np.isfinite(packed).all()
    assert np.array_equal(padded.view(np.uint32), packed.view(np.uint32)), "padded batch against packed batch"
    assert np.array_equal(alone.view(np.uint32), packed.view(np.uint32)), "each sequence alone against the packed batch"
    for b, n in enumerate(S.RAGGED_LENS):    # ... and every hidden state, not only their mean
        assert np.array_equal(hidden_alone[b].view(np.uint32), np.ascontiguousarray(hidden[b, :n]).view(np.uint32)), f"sequence {b} of {n} tokens"


def test_the_switch_moves_attention_and_zero_is_the_kernel_of_before():
    ids, types, mask = S.ragged_batch()
    live = mask.astype(bool)
    enc = _load("h192")
    try:
        unset = enc.hidden_ids(ids, types, mask)[live]
        with _env("MRK_ENCODER_SPLIT_ATTENTION", "0"):
            off = enc.hidden_ids(ids, types, mask)[live]
        with _env("MRK_ENCODER_SPLIT_ATTENTION", "1"):
            on = enc.hidden_ids(ids, types, mask)[live]
    finally:
        enc.close()
    assert np.array_equal(off.view(np.uint32), unset.view(np.uint32)), "switch 0 against the variable unset"
    assert not np.array_equal(on.view(np.uint32), off.view(np.uint32)), "switch 1 ran the attention of switch 0"
    np.testing.assert_allclose(on, off, rtol=0, atol=S.ATOL_F32_HIDDEN)
