"""The encoder over the whole shape range mrk_encoder_load accepts, in both precisions, against oracle/bert.py and against itself.

Which test launches what (csrc/encoder.hip: launch_gemm, launch_gemm_f32, forward_impl; shapes in encoder_shapes.CASES):
  * attention_f32_mfma_kernel<64>, attention_kernel<64> with 1 and 12 heads: test_ragged_batch_against_the_oracle[h64 | h768 | h1024];
    attention_f32_kernel with DH = 64: test_f32_vector_unit_twin[h64 | h768 | h1024];
  * head groups (ATT_HEADS = 4): 1 head h64, 4 + 2 heads h192, 8 groups h1024w - every test of those cases;
  * gemm_skinny_kernel / gemm_f32_skinny_kernel with K / 64 = 8, 12, 16 (h512, h768, h1024 / h1024w), MT = 1 and 2, and the
    `default: return false` fallback to the 64 x 64 tiles at K / 64 = 3, 5 (h192) and 48 (h768): test_one_sequence_alone_has_its_bits_in_the_batch,
    which also sets MRK_ENCODER_SKINNY=0;
  * layer_norm_row with 1, 3, 8, 12 and 16 elements per lane: every test of h64, h192, h512, h768, h1024;
  * gemm_kernel<2, 2> and gemm_f32_mfma32_kernel at K = 512, 768, 1024, 3072 and 64: test_128_tiles_give_the_ragged_bits;
  * attention_kernel (fp16) on masks that are not a prefix, head sizes 32 and 64; attention_f32_mfma_kernel<64> on the same:
    test_masks_with_holes.
Tolerances: encoder_shapes (the encoder suite's own bars); every bit-for-bit check takes none.  Worst errors are printed (pytest -s).
"""
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
CASE_MODE = [(c, m) for c in S.CASES for m in S.MODES]


def _load(case, mode):
    tj = synth.wordpiece_tokenizer_json(vocab_size=S.VOCAB, max_length=S.MAX_POS)
    return HipEncoder(synth.bert_safetensors(S.model(case), S.CASES[case]["heads"]), tj, precision=mode)


@contextlib.contextmanager
def _switch(name, value):
    os.environ[name] = value
    N.reload_switches()
    try:
        yield
    finally:
        del os.environ[name]
        N.reload_switches()


@pytest.mark.parametrize("case,mode", CASE_MODE)
def test_ragged_batch_against_the_oracle(case, mode):
    """Hidden states at live positions against the oracle of the handle's arithmetic; the pooled embedding (packed path) is the
    f64 mean of those very hidden states; the pair logit (packed path) against the oracle's."""
    ids, types, mask = S.ragged_batch()
    heads, fp16, live = S.CASES[case]["heads"], mode == "f16", mask.astype(bool)
    want = S.oracle_hidden(case, mode)
    want_logits = bert.cross_logits(S.model(case), ids, types, mask, heads=heads, fp16=fp16)
    enc = _load(case, mode)
    try:
        assert (enc.info["hidden"], enc.info["heads"], enc.info["intermediate"], enc.info["layers"]) == \
               (S.CASES[case]["hidden"], heads, S.CASES[case]["inter"], S.LAYERS)
        h = enc.hidden_ids(ids, types, mask)
        pooled = enc.embed_ids(ids, types, mask)
        logits = enc.score_ids(ids, types, mask)
    finally:
        enc.close()
    err, lerr = float(np.abs(h - want)[live].max()), float(np.abs(logits - want_logits).max())
    print(f"\n{case} {mode}: hidden |device - oracle| max {err:.3e} (bound {S.atol(case, mode):.1e}), logits {lerr:.3e}", end="")
    assert np.isfinite(h[live]).all()
    np.testing.assert_allclose(h[live], want[live], rtol=0, atol=S.atol(case, mode))
    np.testing.assert_array_equal(pooled, bert.avgpool(h, mask))
    np.testing.assert_allclose(logits, want_logits, rtol=0, atol=S.ATOL_MODEL if fp16 else S.ATOL_F32_LOGIT)


@pytest.mark.parametrize("case,mode", CASE_MODE)
def test_one_sequence_alone_has_its_bits_in_the_batch(case, mode):
    """Each of the nine sequences alone (1 ... 70 rows: the <= 64-row kernels with MT = 1 and 2, their fallback where K / 64 has no
    instantiation, 64 x 64 tiles above) gives the bits of its row in the batch (630 rows: 64 x 64 tiles).  fp16: the same again
    with MRK_ENCODER_SKINNY=0, where the tiles take the one-request products too."""
    ids, types, mask = S.ragged_batch()
    enc = _load(case, mode)
    try:
        ragged = enc.hidden_ids(ids, types, mask)
        def alone():
            return [enc.hidden_ids(ids[b:b + 1, :n], types[b:b + 1, :n], np.ones((1, n), dtype=np.int32)) for b, n in enumerate(S.RAGGED_LENS)]
        got = alone()
        if mode == "f16":
            with _switch("MRK_ENCODER_SKINNY", "0"):
                tiles = alone()
    finally:
        enc.close()
    for b, n in enumerate(S.RAGGED_LENS):
        np.testing.assert_array_equal(got[b][0], ragged[b, :n], err_msg=f"sequence {b} of {n} tokens")
        if mode == "f16":
            np.testing.assert_array_equal(tiles[b][0], ragged[b, :n], err_msg=f"sequence {b} of {n} tokens, MRK_ENCODER_SKINNY=0")


# csrc/encoder.hip, launch_gemm:      const bool big = N % 128 == 0 && (size_t)((M + 127) / 128) * (N / 128) >= 256;
# csrc/encoder.hip, launch_gemm_f32:  const bool big = N % 128 == 0 && (size_t)((M + 127) / 128) * (N / 128) >= 512;
BIG_TILES = {"f16": 256, "f32": 512}


def _repeats(hidden, mode):
    """the fewest copies of the ragged batch whose N = hidden products take 128 x 128 tiles, with a ragged last row tile"""
    rows = len(S.RAGGED_LENS) * S.RAGGED_SEQ
    reps = 1
    while -(-reps * rows // 128) * (hidden // 128) < BIG_TILES[mode] or reps * rows % 128 == 0:
        reps += 1
    return reps


@pytest.mark.parametrize("case,mode", [(c, m) for c in S.TILE128_CASES for m in S.MODES])
def test_128_tiles_give_the_ragged_bits(case, mode):
    """gemm_kernel<2, 2> / gemm_f32_mfma32_kernel: the ragged batch repeated until every product whose N is a multiple of 128
    (N = hidden: the smallest of them) is past launch_gemm's / launch_gemm_f32's threshold; M is no multiple of 128."""
    ids, types, mask = S.ragged_batch()
    reps = _repeats(S.CASES[case]["hidden"], mode)
    M = reps * ids.size
    assert M % 128 != 0 and -(-M // 128) * (S.CASES[case]["hidden"] // 128) >= BIG_TILES[mode] and M < 17000
    enc = _load(case, mode)
    try:
        ragged = enc.hidden_ids(ids, types, mask)
        many = enc.hidden_ids(np.tile(ids, (reps, 1)), np.tile(types, (reps, 1)), np.tile(mask, (reps, 1)))
    finally:
        enc.close()
    np.testing.assert_array_equal(many[:len(ids)], ragged)
    assert np.isfinite(many[np.tile(mask, (reps, 1)).astype(bool)]).all()
    last = many[-len(ids):]          # the copy in the ragged last row tile: the same bits too
    np.testing.assert_array_equal(last[mask.astype(bool)], ragged[mask.astype(bool)])


@pytest.mark.parametrize("case", list(S.CASES))
def test_f32_vector_unit_twin(case):
    """MRK_ENCODER_F32_MFMA=0: gemm_f32_kernel and attention_f32_kernel.  One-token sequences have a softmax of exactly 1.0 in both
    attention kernels, so every product's bits are compared at this case's K; the ragged batch then differs through the two
    attention kernels' softmax bookkeeping only."""
    ids, types, mask = S.ragged_batch()
    live = mask.astype(bool)
    one_ids = np.random.default_rng(3).integers(5, S.VOCAB, size=(300, 1)).astype(np.int32)
    ones = np.ones((300, 1), dtype=np.int32)
    enc = _load(case, "f32")
    try:
        mfma, mfma_one = enc.hidden_ids(ids, types, mask), enc.hidden_ids(one_ids, None, ones)
        with _switch("MRK_ENCODER_F32_MFMA", "0"):
            valu, valu_one = enc.hidden_ids(ids, types, mask), enc.hidden_ids(one_ids, None, ones)
    finally:
        enc.close()
    np.testing.assert_array_equal(valu_one, mfma_one)
    assert np.isfinite(mfma_one).all()
    print(f"\n{case}: f32 attention twins differ by {float(np.abs(valu - mfma)[live].max()):.3e}", end="")
    np.testing.assert_allclose(valu[live], mfma[live], rtol=0, atol=S.ATOL_F32_TWINS)


@pytest.mark.parametrize("case,mode", [(c, m) for c in S.HOLES_CASES for m in S.MODES])
def test_masks_with_holes(case, mode):
    """Whole 32-key blocks of dead keys before the first live key, in the middle and at the end; one live key, the last.  The fp16
    attention_kernel gives the keys of a leading dead block weight exp(0) and lets the first live block's alpha = 0 erase them."""
    ids, types, mask = S.holes_batch()
    live = mask.astype(bool)
    want = S.oracle_hidden(case, mode, "holes")
    enc = _load(case, mode)
    try:
        h = enc.hidden_ids(ids, types, mask)
    finally:
        enc.close()
    print(f"\n{case} {mode}: holes |device - oracle| max {float(np.abs(h - want)[live].max()):.3e} (bound {S.atol(case, mode):.1e})", end="")
    assert np.isfinite(h[live]).all()
    np.testing.assert_allclose(h[live], want[live], rtol=0, atol=S.atol(case, mode))
