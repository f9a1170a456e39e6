"""Encoder models over the whole shape range mrk_encoder_load accepts (head size 32 or 64, widths multiple of 64, hidden <= 1024),
the batches they are run on, and two ways of telling how far apart "right" and "subtly wrong" are - shared by
test_encoder_shapes_cpu.py and test_encoder_shapes_gpu.py.

Nothing here touches the oracle's code: `mutants` and `permuted` change WEIGHTS and MASKS only, oracle/bert.py computes.
  * `mutants`: the model a kernel with one plausible defect would compute - a product that loses its last 16 k, a softmax that
    loses a sequence's last key.  The CPU file requires every one of them to stand at least 4 x the GPU test's tolerance away
    from the oracle, so the GPU comparison does tell right from wrong at these shapes.
  * `permuted`: the same function with the hidden and intermediate axes renumbered - every sum runs over the same terms in
    another order.  Its distance from the plain run is the oracle's own summation-order noise, the floor under any tolerance.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import bert
from workloads import synth

# tests/test_encoder_gpu.py's bars (test_encoder_shapes_cpu.py checks that they still are): the device against the oracle run
# with the device's rounding points (fp16 handle), and against the fp32 graph (f32 handle)
ATOL_MODEL, ATOL_F32_HIDDEN = 4e-3, 2e-4
ATOL_F32_TWINS = 1e-5      # attention_f32_mfma_kernel against attention_f32_kernel: softmax bookkeeping only
ATOL_F32_LOGIT = 5e-4      # test_f32_mode_reproduces_the_fp32_graph's figure for score_ids
ATOL_CAP = 1e-2            # no bound may move past this: the weakest mutant stands 4.3e-2 away
MODES = ("f16", "f32")

# name: hidden, heads, intermediate, bound per mode.  K / 64 of the four products is hidden / 64 (QKV, attention output, FFN 1) and
# intermediate / 64 (FFN 2); the <= 64-row kernels exist for 1, 2, 4, 6, 8, 12, 16, 24, everything else falls through to the tiles.
CASES = {
    # one head (three of a workgroup's four wavefronts leave); f32 head size 64; the smallest legal model; K / 64 = 1
    "h64": dict(hidden=64, heads=1, inter=64, atol={"f16": ATOL_MODEL, "f32": ATOL_F32_HIDDEN}),
    # K / 64 = 3 and 5: the fallback of a one-request product; heads 4 + 2; no N divisible by 128; LayerNorm 3 per lane
    "h192": dict(hidden=192, heads=6, inter=320, atol={"f16": ATOL_MODEL, "f32": ATOL_F32_HIDDEN}),
    # K / 64 = 8
    "h512": dict(hidden=512, heads=16, inter=512, atol={"f16": ATOL_MODEL, "f32": ATOL_F32_HIDDEN}),
    # BERT-base: K / 64 = 12, and 48 (fallback); f32 head size 64
    "h768": dict(hidden=768, heads=12, inter=3072, atol={"f16": ATOL_MODEL, "f32": ATOL_F32_HIDDEN}),
    # K / 64 = 16; LayerNorm 16 per lane (LN_MAX_PER_LANE)
    "h1024": dict(hidden=1024, heads=16, inter=1024, atol={"f16": ATOL_MODEL, "f32": ATOL_F32_HIDDEN}),
    # eight head groups; intermediate narrower than hidden (FFN 1 has N = 64, FFN 2 has K / 64 = 1)
    "h1024w": dict(hidden=1024, heads=32, inter=64, atol={"f16": ATOL_MODEL, "f32": ATOL_F32_HIDDEN}),
}
TILE128_CASES = ("h512", "h768", "h1024", "h1024w")   # hidden divisible by 128
HOLES_CASES = ("h192", "h64", "h768")
VOCAB, MAX_POS, LAYERS = 300, 80, 2

# On both sides of the 16-key block of f32 attention, the 32-key block of fp16 attention, the <= 16 / <= 32 rows of the f32
# skinny kernel and the <= 32 / <= 64 rows of the fp16 one
RAGGED_LENS = (70, 1, 16, 17, 31, 32, 33, 64, 65)
RAGGED_SEQ = 70


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def model(case: str) -> dict:
    c = CASES[case]
    w = synth.synthetic_bert(layers=LAYERS, vocab=VOCAB, max_pos=MAX_POS, seed=4, classifier=True, hidden=c["hidden"], heads=c["heads"], inter=c["inter"])
    return {k: _frozen(v) for k, v in w.items()}


def atol(case: str, mode: str) -> float:
    return CASES[case]["atol"][mode]


@functools.lru_cache(maxsize=None)
def ragged_batch():
    """ids, type ids, mask: nine sequences of RAGGED_LENS in 70 columns, type 1 from position 35 on"""
    rng = np.random.default_rng(20261020)
    n = len(RAGGED_LENS)
    ids = rng.integers(5, VOCAB, size=(n, RAGGED_SEQ)).astype(np.int32)
    types = np.zeros_like(ids)
    types[:, 35:] = 1
    mask = (np.arange(RAGGED_SEQ)[None, :] < np.array(RAGGED_LENS)[:, None]).astype(np.int32)
    return _frozen(ids), _frozen(types), _frozen(mask)


@functools.lru_cache(maxsize=None)
def holes_batch():
    """Masks that are not a prefix of ones, cut along the fp16 kernel's 32-key blocks (test_encoder_gpu.py has the 16-key ones)"""
    rng = np.random.default_rng(20261021)
    n, seq = 5, 80
    ids = rng.integers(5, VOCAB, size=(n, seq)).astype(np.int32)
    types = np.zeros_like(ids)
    mask = np.zeros((n, seq), dtype=np.int32)
    mask[0, 64:76] = 1                      # two dead blocks, then live keys, then dead to the end
    mask[1, 32:] = 1                        # exactly one dead block first
    mask[2, :20] = 1; mask[2, 64:70] = 1    # a dead block in the middle
    mask[3, 79] = 1                         # one live key, the last
    mask[4, :] = 1
    return _frozen(ids), _frozen(types), _frozen(mask)


BATCHES = {"ragged": ragged_batch, "holes": holes_batch}


@functools.lru_cache(maxsize=None)
def oracle_hidden(case: str, mode: str, batch: str = "ragged"):
    """The reference of a (case, precision, batch), computed once per process and read-only: the oracle with the device's
    rounding points for an fp16 handle, the fp32 graph for an f32 one."""
    ids, types, mask = BATCHES[batch]()
    return _frozen(bert.last_hidden_state(model(case), ids, types, mask, heads=CASES[case]["heads"], fp16=(mode == "f16")))


MUTANT_WEIGHTS = ("attention.self.query", "attention.self.value", "attention.output.dense", "intermediate.dense", "output.dense")


def mutants(w: dict, mask):
    """(label, weights, mask) of six wrong models: the last layer's Q, V, attention-output, FFN-1 and FFN-2 weight with the last
    16 input columns zeroed (a product that stops 16 k early), one at a time; and the mask with every sequence's last live key
    cleared (a softmax that stops one key early)."""
    last = bert.n_layers(w) - 1
    for nm in MUTANT_WEIGHTS:
        key = f"encoder.layer.{last}.{nm}.weight"
        cut = w[key].copy()
        cut[:, -16:] = 0
        yield nm, {**w, key: cut}, mask
    short = np.array(mask, copy=True)
    for b in range(short.shape[0]):
        short[b, np.flatnonzero(short[b])[-1]] = 0
    yield "last live key", w, short


def permuted(w: dict, seed: int):
    """(weights, perm): the same function with hidden channel i of the result at perm's position, i.e. result[..., j] is the
    plain model's [..., perm[j]].  One permutation of the hidden axis goes to the embedding columns, every LayerNorm's
    parameters, the input dimensions of Q, K, V, FFN-1 and the pooler, the output dimensions and biases of attention-output and
    FFN-2; another one renumbers the intermediate axis (FFN-1's outputs, FFN-2's inputs).  Heads stay whole: Q / K / V outputs
    and attention-output's inputs are not touched."""
    rng = np.random.default_rng(seed)
    H = w["embeddings.word_embeddings.weight"].shape[1]
    I = w["encoder.layer.0.intermediate.dense.weight"].shape[0]
    p, r = rng.permutation(H), rng.permutation(I)
    out = dict(w)
    cols = lambda k: out.__setitem__(k, np.ascontiguousarray(w[k][:, p]))
    rows = lambda k: out.__setitem__(k, np.ascontiguousarray(w[k][p]))
    def norm(name):
        rows(name + ".weight"); rows(name + ".bias")
    for k in ("word_embeddings", "position_embeddings", "token_type_embeddings"):
        cols(f"embeddings.{k}.weight")
    norm("embeddings.LayerNorm")
    for l in range(bert.n_layers(w)):
        q = f"encoder.layer.{l}."
        for nm in ("query", "key", "value"):
            cols(q + f"attention.self.{nm}.weight")
        rows(q + "attention.output.dense.weight"); rows(q + "attention.output.dense.bias")
        norm(q + "attention.output.LayerNorm")
        out[q + "intermediate.dense.weight"] = np.ascontiguousarray(w[q + "intermediate.dense.weight"][r][:, p])
        out[q + "intermediate.dense.bias"] = np.ascontiguousarray(w[q + "intermediate.dense.bias"][r])
        out[q + "output.dense.weight"] = np.ascontiguousarray(w[q + "output.dense.weight"][p][:, r])
        rows(q + "output.dense.bias")
        norm(q + "output.LayerNorm")
    if "pooler.dense.weight" in w:
        cols("pooler.dense.weight")
    return out, p


def order_noise(case: str, mode: str, seeds=(1, 2, 3)) -> float:
    """max over `seeds` of |permuted run - plain run| at the ragged batch's live positions: the oracle against itself"""
    ids, types, mask = ragged_batch()
    live = mask.astype(bool)
    plain = oracle_hidden(case, mode)
    worst = 0.0
    for seed in seeds:
        w2, p = permuted(model(case), seed)
        h = bert.last_hidden_state(w2, ids, types, mask, heads=CASES[case]["heads"], fp16=(mode == "f16"))
        worst = max(worst, float(np.abs(h[live] - plain[..., p][live]).max()))
    return worst
