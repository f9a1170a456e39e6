"""GPU: the split-bf16 encoder precision (MRK_ENCODER_SPLIT, csrc/encoder_split.hip) - the dense products as three bf16 products of
two-term splits, f32 accumulation.  Held to the f32 handle's own bars against the fp32 graph (encoder_shapes), and to the f32
handle's load independence: one accumulation order per output element, so the same bits in every launch shape.

Launch shapes of gemm_split_kernel (launch_gemm_split): <= 32 rows -> 32 x 64 tiles of two wavefronts; more -> 64 x 64 tiles; N % 128
== 0 with >= 256 tiles of 128 x 128 -> those.  The ragged batch's lengths lie on both sides of 32 rows; test_128_tiles reaches the third.
K / 64 = 1 (h64), 3 and 5 (h192, no N divisible by 128), 12 and 48 (h768)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import encoder_shapes as S
import semantic_cases
from metarank_amd import _native as N
from metarank_amd.encoder import HipEncoder
from metarank_amd.index import HipIndex
from oracle import bert
from workloads import synth

pytestmark = pytest.mark.gpu
CASES = ("h64", "h192", "h768")


def _load(case, mode="split"):
    tj = synth.wordpiece_tokenizer_json(vocab_size=S.VOCAB, max_length=S.MAX_POS)
    return HipEncoder(synth.bert_safetensors(S.model(case), S.CASES[case]["heads"]), tj, precision=mode)


@contextlib.contextmanager
def _padded():
    os.environ["MRK_ENCODER_PACKED"] = "0"
    N.reload_switches()
    try:
        yield
    finally:
        del os.environ["MRK_ENCODER_PACKED"]
        N.reload_switches()


@pytest.mark.parametrize("case,batch", [(c, b) for c in CASES for b in S.BATCHES])
def test_within_the_f32_bars_of_the_fp32_graph(case, batch):
    """hidden states at live positions against the fp32 graph, bound ATOL_F32_HIDDEN; pair logits of the ragged batch, ATOL_F32_LOGIT"""
    ids, types, mask = S.BATCHES[batch]()
    live = mask.astype(bool)
    want = S.oracle_hidden(case, "f32", batch)
    enc = _load(case)
    try:
        h = enc.hidden_ids(ids, types, mask)
        logits = enc.score_ids(ids, types, mask) if batch == "ragged" else None
    finally:
        enc.close()
    print(f"\n{case} {batch}: hidden |split - fp32 graph| max {float(np.abs(h - want)[live].max()):.3e} (bound {S.ATOL_F32_HIDDEN:.1e})", end="")
    assert np.isfinite(h[live]).all()
    np.testing.assert_allclose(h[live], want[live], rtol=0, atol=S.ATOL_F32_HIDDEN)
    if logits is not None:
        want_logits = bert.cross_logits(S.model(case), ids, types, mask, heads=S.CASES[case]["heads"], fp16=False)
        print(f", logits {float(np.abs(logits - want_logits).max()):.3e} (bound {S.ATOL_F32_LOGIT:.1e})", end="")
        np.testing.assert_allclose(logits, want_logits, rtol=0, atol=S.ATOL_F32_LOGIT)


@pytest.mark.parametrize("case", ["h192", "h768"])
def test_a_sequence_has_the_same_bits_alone_padded_and_packed(case):
    ids, types, mask = S.ragged_batch()
    enc = _load(case)
    try:
        packed = enc.embed_ids(ids, types, mask)
        with _padded():
            padded = enc.embed_ids(ids, types, mask)
        alone = np.concatenate([enc.embed_ids(ids[b:b + 1, :n], types[b:b + 1, :n], np.ones((1, n), dtype=np.int32)) for b, n in enumerate(S.RAGGED_LENS)])
        hidden = enc.hidden_ids(ids, types, mask)
        hidden_alone = [enc.hidden_ids(ids[b:b + 1, :n], types[b:b + 1, :n], np.ones((1, n), dtype=np.int32))[0] for b, n in enumerate(S.RAGGED_LENS)]
    finally:
        enc.close()
    assert np.isfinite(packed).all()
    np.testing.assert_array_equal(padded, packed)
    np.testing.assert_array_equal(alone, packed)
    for b, n in enumerate(S.RAGGED_LENS):    # ... and every hidden state, not only their mean
        np.testing.assert_array_equal(hidden_alone[b], hidden[b, :n], err_msg=f"sequence {b} of {n} tokens")


def test_128_tiles_give_the_ragged_bits():
    """h768: nine copies of the ragged batch, 5 670 rows = 45 row tiles of 128 (the last one ragged) x 6 column tiles >= 256"""
    ids, types, mask = S.ragged_batch()
    reps = 9
    assert (reps * ids.size) % 128 != 0 and -(-reps * ids.size // 128) * (768 // 128) >= 256
    enc = _load("h768")
    try:
        ragged = enc.hidden_ids(ids, types, mask)
        many = enc.hidden_ids(np.tile(ids, (reps, 1)), np.tile(types, (reps, 1)), np.tile(mask, (reps, 1)))
    finally:
        enc.close()
    live = mask.astype(bool)
    np.testing.assert_array_equal(many[:len(ids)][live], ragged[live])
    np.testing.assert_array_equal(many[-len(ids):][live], ragged[live])


def test_an_index_row_has_the_bits_of_the_text_alone(ctx):
    gold = semantic_cases.GOLDEN
    enc = HipEncoder(open(os.path.join(gold, "encoder_tiny.onnx"), "rb").read(), open(os.path.join(gold, "tokenizer_tiny.json"), "rb").read(), ctx=ctx, precision="split")
    try:
        ids, texts = semantic_cases.catalogue()
        alone = np.concatenate([enc.embed([t]) for t in texts])
        ix = HipIndex.fit_semantic(enc, ids, texts, max_tokens=37)   # ~70 pieces
        v = ix.vectors()
        ix.close()
    finally:
        enc.close()
    assert np.array_equal(v.view(np.uint64), alone.astype(np.float64).view(np.uint64))


def test_the_mode_is_taken_and_other_values_are_refused(ctx):
    """split and f32 handles on one model: not the same bits, yet within ATOL_F32_HIDDEN; precision 4 stays MRK_ERR_INVALID_ARG"""
    ids, types, mask = S.ragged_batch()
    got = {}
    for mode in ("split", "f32"):
        enc = _load("h192", mode)
        try:
            got[mode] = enc.embed_ids(ids, types, mask)
        finally:
            enc.close()
    assert not np.array_equal(got["split"].view(np.uint32), got["f32"].view(np.uint32))
    np.testing.assert_allclose(got["split"], got["f32"], rtol=0, atol=S.ATOL_F32_HIDDEN)
    blob = synth.bert_safetensors(S.model("h64"), 1)
    tj = synth.wordpiece_tokenizer_json(vocab_size=S.VOCAB, max_length=S.MAX_POS).encode()
    out = C.c_void_p()
    assert N.lib().mrk_encoder_load_ex(ctx.handle, blob, len(blob), tj, len(tj), 0, 4, C.byref(out)) == N.ERR_INVALID_ARG and not out.value
