"""What the GPU comparison of test_encoder_shapes_gpu.py is worth, settled on the CPU: at every shape of encoder_shapes.CASES and
in both oracle modes, (1) a model with one plausible kernel defect stands at least 4 x the GPU test's tolerance away from the
oracle, and (2) the oracle's own summation-order noise stays below that tolerance.  Figures are printed (pytest -s)."""
import numpy as np
import pytest

import encoder_shapes as S
from oracle import bert

CASE_MODE = [(c, m) for c in S.CASES for m in S.MODES]


def test_the_bars_are_the_encoder_suites_own():
    import test_encoder_gpu as E
    assert (S.ATOL_MODEL, S.ATOL_F32_HIDDEN) == (E.ATOL_MODEL, E.ATOL_F32_HIDDEN)
    for case, c in S.CASES.items():
        # a bound that moved is 2 x the order noise measured below, and never past the cap
        assert S.ATOL_F32_HIDDEN == c["atol"]["f32"] and S.ATOL_MODEL <= c["atol"]["f16"] <= S.ATOL_CAP, case
        dh = c["hidden"] // c["heads"]
        assert dh * c["heads"] == c["hidden"] and dh in (32, 64) and c["hidden"] % 64 == 0 and c["inter"] % 64 == 0 and c["hidden"] <= 1024


def test_permuted_is_a_symmetry_of_the_model():
    """The embedding sum (no reduction yet) is the plain one with its channels renumbered, bit for bit; the pair logits - which the
    renumbering does not reach, the pooler's inputs being renumbered with it - agree to f32 summation order."""
    w = S.model("h192")
    ids, types, mask = S.ragged_batch()
    w2, p = S.permuted(w, 7)
    assert sorted(p.tolist()) == list(range(192)) and not np.array_equal(p, np.arange(192))
    emb = lambda v: v["embeddings.word_embeddings.weight"][ids] + v["embeddings.token_type_embeddings.weight"][types]
    np.testing.assert_array_equal(emb(w2), emb(w)[..., p])
    a = bert.cross_logits(w, ids, types, mask, heads=6)
    b = bert.cross_logits(w2, ids, types, mask, heads=6)
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-5)


@pytest.mark.parametrize("case,mode", CASE_MODE)
def test_every_mutant_stands_clear_of_the_oracle(case, mode):
    ids, types, mask = S.ragged_batch()
    want = S.oracle_hidden(case, mode)
    tol = S.atol(case, mode)
    for label, w2, m2 in S.mutants(S.model(case), mask):
        h = bert.last_hidden_state(w2, ids, types, m2, heads=S.CASES[case]["heads"], fp16=(mode == "f16"))
        d = np.abs(h - want)
        if m2 is mask:
            seps = [float(d[mask.astype(bool)].max())]
        else:   # per sequence, at the positions still live (the one-token sequence has none left)
            seps = [float(d[b][m2[b].astype(bool)].max()) for b in range(len(m2)) if m2[b].any()]
            assert len(seps) == len(m2) - 1
        print(f"\n{case} {mode} mutant '{label}': separation {min(seps):.3e} (tolerance {tol:.1e})", end="")
        assert min(seps) >= 4 * tol, (label, seps)


@pytest.mark.parametrize("case,mode", CASE_MODE)
def test_order_noise_stays_below_the_tolerance(case, mode):
    noise = S.order_noise(case, mode)
    print(f"\n{case} {mode}: order noise {noise:.3e} (tolerance {S.atol(case, mode):.1e})", end="")
    assert 0.0 < noise < S.atol(case, mode)
