"""Micro-benchmark of the text-encoder leg (all-MiniLM-L6-v2's shape, random weights -- there is no network for
checkpoints and the arithmetic does not depend on the values): single-query latency (the /rank case), batched query
throughput, and a cross-encoder batch (the only MFMA-bound work on the path).  FLOPs = 2 * tokens * matrix parameters
(+ attention 4 * seq * hidden per token per layer), padding tokens included because the kernels compute them.
  python tools/encoder_bench.py [--json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from workloads import synth  # noqa: E402
from metarank_amd.encoder import HipEncoder, HipTokenizer  # noqa: E402


def flops(n, seq, layers=6, H=384, I=1536):
    per_tok = layers * (2 * (4 * H * H + 2 * H * I) + 4 * seq * H)
    return n * seq * per_tok


def timeit(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return np.array(ts)


BF16_PEAK_TFLOPS = 2500.0   # dense bf16 matrix peak of the MI355X


def compare(reps):
    """One packed forward pass (mrk_encoder_embed_ids) in all three precisions, same process, same inputs, the precisions taken in
    turn inside every repetition: HIP events around the forward pass (mrk_profile_enable's "encoder" timer), median of `reps`.
    split_product_tflops = the bf16 work of the dense products (SPLIT_PRODUCTS = 3 products of 2 M N K each) over the WHOLE pass -
    a lower bound of the split kernel's own rate; the kernel's share of peak comes from a kernel trace of --precision split."""
    import metarank_amd as M
    ctx = M.Context(0)
    ctx.profile_enable(True)
    out = {}
    rng = np.random.default_rng(9)
    for name, shape, n, lo, hi in (("minilm_c5_batch", dict(layers=6, hidden=384, heads=12, inter=1536), 3840, 0, 0),
                                   ("bert_base_384_tokens", dict(layers=12, hidden=768, heads=12, inter=3072), 12, 16, 48)):
        tj = synth.wordpiece_tokenizer_json(vocab_size=2000, max_length=128)
        blob = synth.bert_safetensors(synth.synthetic_bert(**shape), shape["heads"])
        if lo:   # n sequences of lo .. hi random tokens
            lens = rng.integers(lo, hi + 1, size=n); lens[0] = hi
            ids = rng.integers(5, 2000, size=(n, hi)).astype(np.int32); ty = np.zeros_like(ids)
            m = (np.arange(hi)[None, :] < lens[:, None]).astype(np.int32)
        else:    # bench.py --workload c5: one device batch's queries
            ids, ty, m = HipTokenizer(tj).encode_batch(synth.synthetic_queries(n, seed=3))
        encs = {p: HipEncoder(blob, tj, ctx=ctx, precision=p) for p in ("f32", "f16", "split")}
        ms = {p: [] for p in encs}
        emb = {}
        for r in range(3 + reps):
            for p, e in encs.items():
                t0 = ctx.profile_get("encoder")[0]
                emb[p] = e.embed_ids(ids, ty, m)
                if r >= 3:
                    ms[p].append(ctx.profile_get("encoder")[0] - t0)
        tokens, H, I, L = int(m.sum()), shape["hidden"], shape["inter"], shape["layers"]
        dense = 2.0 * tokens * L * (4 * H * H + 2 * H * I)
        med = {p: float(np.median(v)) for p, v in ms.items()}
        out[name] = {"tokens": tokens, "sequences": int(n), "ms": med, "ms_min_max": {p: [float(min(v)), float(max(v))] for p, v in ms.items()},
                     "split_vs_f32_time": med["split"] / med["f32"], "split_product_tflops_whole_pass": 3 * dense / med["split"] / 1e9,
                     "frac_of_bf16_peak_whole_pass": 3 * dense / med["split"] / 1e9 / BF16_PEAK_TFLOPS,
                     "max_abs_embedding_diff_vs_f32": {p: float(np.abs(emb[p] - emb["f32"]).max()) for p in ("f16", "split")}}
        for e in encs.values():
            e.close()
    out["ranking_vs_f32"] = rank_agreement(ctx)
    ctx.close()
    return out


SINGLE_SHAPES = {"minilm_l6": dict(layers=6, hidden=384, heads=12, inter=1536), "bert_base": dict(layers=12, hidden=768, heads=12, inter=3072)}


def single(reps, shapes):
    """One request's query - ONE sequence of 9 and of 32 tokens - on an f32 handle and on a split handle with MRK_ENCODER_SPLIT_SKINNY=0
    (the 32 x 64 tile) and =1 (gemm_split_skinny_kernel): same process, the three taken in turn inside every repetition, HIP events
    around the forward pass (the "encoder" timer), 3 warm-ups, median [min, max] in ms.  The two split runs must give the same bits."""
    import metarank_amd as M
    from metarank_amd import _native
    ctx = M.Context(0)
    ctx.profile_enable(True)
    rng = np.random.default_rng(9)
    tj = synth.wordpiece_tokenizer_json(vocab_size=2000, max_length=128)
    out = {}
    for name in shapes:
        shape = SINGLE_SHAPES[name]
        blob = synth.bert_safetensors(synth.synthetic_bert(**shape), shape["heads"])
        encs = {"f32": HipEncoder(blob, tj, ctx=ctx, precision="f32"), "split": HipEncoder(blob, tj, ctx=ctx, precision="split")}
        for n in (9, 32):
            ids = rng.integers(5, 2000, size=(1, n)).astype(np.int32); ty = np.zeros_like(ids); m = np.ones_like(ids)
            runs = (("f32", "f32", None), ("split_tile", "split", "0"), ("split_skinny", "split", "1"))
            ms, emb = {r[0]: [] for r in runs}, {}
            for r in range(3 + reps):
                for key, handle, switch in runs:
                    if switch is not None:
                        os.environ["MRK_ENCODER_SPLIT_SKINNY"] = switch
                        _native.reload_switches()
                    t0 = ctx.profile_get("encoder")[0]
                    emb[key] = encs[handle].embed_ids(ids, ty, m)
                    if r >= 3:
                        ms[key].append(ctx.profile_get("encoder")[0] - t0)
            os.environ.pop("MRK_ENCODER_SPLIT_SKINNY", None)
            _native.reload_switches()
            out[f"{name}_{n}_tokens"] = {"ms": {k: float(np.median(v)) for k, v in ms.items()}, "ms_min_max": {k: [float(min(v)), float(max(v))] for k, v in ms.items()},
                                         "skinny_vs_tile_time": float(np.median(ms["split_skinny"]) / np.median(ms["split_tile"])),
                                         "same_bits_skinny_and_tile": bool(np.array_equal(emb["split_skinny"].view(np.uint32), emb["split_tile"].view(np.uint32))),
                                         "max_abs_embedding_diff_vs_f32": float(np.abs(emb["split_skinny"] - emb["f32"]).max())}
        for e in encs.values():
            e.close()
    ctx.close()
    return out


ATTENTION_TOKENS = 8192   # tokens of a batch of attention(): 256 sequences of 32, 64 of 128, 16 of 512


def attention(reps, shapes):
    """A split handle's packed batch of ATTENTION_TOKENS tokens in sequences of 32, 128 and 512 with MRK_ENCODER_SPLIT_ATTENTION=0
    (attention_f32_mfma_kernel) and =1 (attention_split_kernel): same process, the two taken in turn inside every repetition, HIP
    events around the forward pass (the "encoder" timer), 3 warm-ups, median [min, max] in ms."""
    import metarank_amd as M
    from metarank_amd import _native
    ctx = M.Context(0)
    ctx.profile_enable(True)
    rng = np.random.default_rng(9)
    tj = synth.wordpiece_tokenizer_json(vocab_size=2000, max_length=512)
    out = {}
    for name in shapes:
        shape = SINGLE_SHAPES[name]
        enc = HipEncoder(synth.bert_safetensors(synth.synthetic_bert(**shape), shape["heads"]), tj, ctx=ctx, precision="split")
        for seq in (32, 128, 512):
            ids = rng.integers(5, 2000, size=(ATTENTION_TOKENS // seq, seq)).astype(np.int32); ty = np.zeros_like(ids); m = np.ones_like(ids)
            ms, emb = {"0": [], "1": []}, {}
            for r in range(3 + reps):
                for switch in ms:
                    os.environ["MRK_ENCODER_SPLIT_ATTENTION"] = switch
                    _native.reload_switches()
                    t0 = ctx.profile_get("encoder")[0]
                    emb[switch] = enc.embed_ids(ids, ty, m)
                    if r >= 3:
                        ms[switch].append(ctx.profile_get("encoder")[0] - t0)
            os.environ.pop("MRK_ENCODER_SPLIT_ATTENTION", None)
            _native.reload_switches()
            out[f"{name}_{seq}_tokens"] = {"sequences": int(ids.shape[0]), "ms": {k: float(np.median(v)) for k, v in ms.items()},
                                           "ms_min_max": {k: [float(min(v)), float(max(v))] for k, v in ms.items()},
                                           "switch_1_vs_0_time": float(np.median(ms["1"]) / np.median(ms["0"])),
                                           "max_abs_embedding_diff_1_vs_0": float(np.abs(emb["1"] - emb["0"]).max())}
        enc.close()
    ctx.close()
    return out


def rank_agreement(ctx, requests=96, items=100, catalogue=5000, sessions=500, trees=500):
    """bench.py's config 5 in small (24 Ranklens columns + the bi-encoder cosine, a 500-tree forest): how far an fp16 and a split
    handle move the f32 handle's scores and order - INTEGRATION.md's pair of figures."""
    import itertools
    import metarank_amd as M
    from workloads import ranklens
    ranker = M.HipRanker(ranklens.c5_config(), ctx)
    tj = synth.wordpiece_tokenizer_json(vocab_size=2000, max_length=128)
    blob = synth.bert_safetensors(synth.synthetic_bert(), 12)
    put = {"double": ranker.put_double, "string": ranker.put_string, "string_list": ranker.put_string_list, "double_list": ranker.put_double_list,
           "counter": ranker.put_counter, "periodic": ranker.put_periodic, "bounded_list": ranker.put_bounded_list}
    for kind, key, value in itertools.chain(ranklens.generate_state(catalogue, sessions), ranklens.c5_embeddings(catalogue)):
        put[kind](key, value)
    ranker.flush()
    def with_queries(evs, seed):
        for ev, q in zip(evs, synth.synthetic_queries(len(evs), seed=seed)):
            ev["fields"] = [{"name": "query", "value": q}]
        return evs
    encs = {p: HipEncoder(blob, tj, ctx=ctx, precision=p) for p in ("f32", "f16", "split")}
    ranker.bind_encoder("title_match", encs["f32"])
    sample = ranker.prepare("xgboost", with_queries(ranklens.generate_requests(64, 100, catalogue, sessions, seed=ranklens.SEED + 99), 77))
    sample.run(None)
    _, _, sm = sample.fetch(matrix=True)
    sample.close()
    model = synth.synthetic_lgbm_model(n_trees=trees, n_features=ranker.dim("xgboost"), num_leaves=16, max_depth=8, quantiles=ranklens.column_quantiles(sm, n=49),
                                       missing="per_feature")
    booster = M.HipBooster(model, M.LIGHTGBM, ctx)
    evs = with_queries(ranklens.generate_requests(requests, items, catalogue, sessions, seed=ranklens.SEED + 1), 100)
    res = {}
    for p, e in encs.items():
        ranker.bind_encoder("title_match", e)
        b = ranker.prepare("xgboost", evs)
        b.run(booster)
        s, o, _ = b.fetch()
        res[p] = (s.copy(), o.copy(), list(b.offsets))
        b.close()
    s32, o32, offs = res["f32"]
    out = {"requests": requests, "items": int(len(s32)), "trees": trees}
    for p in ("f16", "split"):
        s, o, _ = res[p]
        out[p] = {"scores_over_1e-5": int((np.abs(s - s32) > 1e-5).sum()), "max_abs_score_diff": float(np.abs(s - s32).max()),
                  "reordered_requests": sum(1 for r in range(requests) if not np.array_equal(o[offs[r]:offs[r + 1]], o32[offs[r]:offs[r + 1]]))}
    booster.close()
    for e in encs.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--precision", choices=["f16", "f32", "split"], default="f16")
    ap.add_argument("--quick", action="store_true", help="single query + the c5 batch (3 840 queries) only")
    ap.add_argument("--compare", type=int, default=0, metavar="REPS", help="f32 / f16 / split side by side (see compare()), nothing else")
    ap.add_argument("--single", type=int, default=0, metavar="REPS", help="one 9- and one 32-token query: f32 / split on the 32 x 64 tile / split on the skinny kernel (see single()), nothing else")
    ap.add_argument("--shape", choices=sorted(SINGLE_SHAPES), default=None, help="--single: this shape only (a kernel trace per shape)")
    ap.add_argument("--attention", type=int, default=0, metavar="REPS", help="a split handle's 8 192-token batch at 32, 128 and 512 tokens a sequence with MRK_ENCODER_SPLIT_ATTENTION=0 and =1 (see attention()), nothing else; --shape as for --single")
    a = ap.parse_args()
    if a.attention:
        print(json.dumps(attention(a.attention, [a.shape] if a.shape else list(SINGLE_SHAPES))))
        return
    if a.single:
        print(json.dumps(single(a.single, [a.shape] if a.shape else list(SINGLE_SHAPES))))
        return
    if a.compare:
        print(json.dumps(compare(a.compare)))
        return
    w = synth.synthetic_bert(classifier=True)
    tj = synth.wordpiece_tokenizer_json(vocab_size=2000, max_length=128)
    enc = HipEncoder(synth.bert_safetensors(w, 12), tj, precision=a.precision)
    tok = HipTokenizer(tj)
    out = {}
    q1 = synth.synthetic_queries(1, seed=1)
    ids, ty, m = tok.encode_batch(q1)
    t = timeit(lambda: enc.embed(q1), 200)
    out["single_query"] = {"tokens": int(m.sum()), "p50_ms": float(np.percentile(t, 50) * 1e3), "p99_ms": float(np.percentile(t, 99) * 1e3)}
    t = timeit(lambda: enc.embed_ids(ids, ty, m), 200)
    out["single_query_ids"] = {"p50_ms": float(np.percentile(t, 50) * 1e3)}
    qs = synth.synthetic_queries(3840, seed=3)   # bench.py --workload c5: one device batch's queries, packed
    ids, ty, m = tok.encode_batch(qs)
    t = timeit(lambda: enc.embed_ids(ids, ty, m), 10)
    ms = float(np.median(t) * 1e3)
    real = int(m.sum())
    out["c5_batch_3840"] = {"tokens": real, "ms": ms, "tflops_real_tokens": sum(flops(1, int(l)) for l in m.sum(axis=1)) / ms / 1e9}
    for n in (() if a.quick else (64, 256, 1024)):
        qs = synth.synthetic_queries(n, seed=2)
        ids, ty, m = tok.encode_batch(qs)
        t = timeit(lambda: enc.embed_ids(ids, ty, m), 20)
        ms = float(np.median(t) * 1e3)
        out[f"queries_{n}"] = {"seq": int(ids.shape[1]), "ms": ms, "queries_per_s": n / ms * 1e3, "tflops": flops(n, ids.shape[1]) / ms / 1e9}
    for n, seq in (() if a.quick else ((100, 64), (100, 128), (1000, 64), (4096, 64))):
        rng = np.random.default_rng(1)
        ids = rng.integers(5, 2000, size=(n, seq)).astype(np.int32); ty = np.zeros_like(ids); m = np.ones_like(ids)
        t = timeit(lambda: enc.score_ids(ids, ty, m), 10)
        ms = float(np.median(t) * 1e3)
        out[f"cross_{n}x{seq}"] = {"ms": ms, "pairs_per_s": n / ms * 1e3, "tflops": flops(n, seq) / ms / 1e9}
    if a.json:
        print(json.dumps(out))
    else:
        for k, v in out.items():
            print(k, {kk: (round(vv, 4) if isinstance(vv, float) else vv) for kk, vv in v.items()})


if __name__ == "__main__":
    main()
