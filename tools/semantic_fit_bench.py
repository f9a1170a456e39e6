"""Measurement of the semantic recommender's fit (mrk_index_build_texts) against what a host has to do
without it: cut the texts into chunks of the same token budget, mrk_encoder_embed per chunk (embeddings to the host), one
mrk_index_build of the concatenated floats (embeddings up again).  Not a test.  One JSON line per case.

Encoder: the MiniLM-L6-shaped synthetic checkpoint and tokenizer of bench.py's c5 workload (workloads/synth.py), f32 handle.
Catalogue (a): --items texts of 4 ... 48 tokens, uniform.  Catalogue (b): the same with 1 % of the texts at the tokenizer's
truncation length.  The two forms run interleaved in this process, `--rounds` each after a warm-up of both.

Per case: wall time and items/s; host tokenisation time (one thread, the whole catalogue, measured on its own); device time of
the forward passes (mrk_profile_get "encoder") and of the pack and the norms (HIP events: "knn_pool_pack", "knn_norms"); the
share of the wall time the device sat idle; device memory held after the call (hipMemGetInfo before and after; the encoder's
scratch is grow-only, so this is the peak).  --sweep: the max_tokens sweep that fixes the library's default.  --sorted: on
catalogue (b), length-ordered windows (MRK_SEMANTIC_WINDOW=4, the default) against input order (=0).
  python tools/semantic_fit_bench.py [--items N] [--rounds K] [--sweep] [--sorted] [--budget T]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import metarank_amd as M  # noqa: E402
from metarank_amd import _native as N  # noqa: E402
from metarank_amd.encoder import HipEncoder, HipTokenizer  # noqa: E402
from metarank_amd.index import HipIndex  # noqa: E402
from workloads import synth  # noqa: E402

MAX_LENGTH = 128     # bench.py c5's tokenizer
ROW_CAP = 65535


def catalogue(tok_json, items, long_share, seed=0):
    """texts whose token counts (with [CLS] / [SEP]) are uniform in 4 ... 48; `long_share` of them at the truncation length.
    Words are whole vocabulary entries, so a text of k words is k + 2 tokens."""
    vocab = json.loads(tok_json)["model"]["vocab"]
    words = np.array([w for w in vocab if len(w) > 2 and not w.startswith(("##", "["))])
    rng = np.random.default_rng(seed)
    lens = rng.integers(4, 49, items)
    if long_share > 0:
        lens[rng.choice(items, int(items * long_share), replace=False)] = MAX_LENGTH
    picks = rng.integers(0, len(words), int(lens.sum() - 2 * items))
    cuts = np.cumsum(lens - 2)[:-1]
    texts = [" ".join(p) for p in np.split(words[picks], cuts)]
    return texts, lens.astype(np.int64)


def strs(vals):
    bs = [v.encode() for v in vals]
    return (C.c_char_p * max(len(bs), 1))(*bs), bs


class Hip:
    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")

    def free_bytes(self):
        free, total = C.c_size_t(), C.c_size_t()
        assert self.lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value


def timers(ctx):
    return {k: ctx.profile_get(k)[0] for k in ("encoder", "knn_pool_pack", "knn_norms")}


def run_new(ctx, enc, pi, pt, n, budget):
    h = C.c_void_p()
    before = timers(ctx)
    t = time.perf_counter()
    N.check(N.lib().mrk_index_build_texts(ctx.handle, enc.handle, pi, pt, n, budget, C.byref(h)))
    wall = time.perf_counter() - t
    after = timers(ctx)
    return HipIndex(h, ctx), wall, {k: after[k] - before[k] for k in after}


def run_parent(ctx, enc, pi, pt, n, lens, budget):
    """the parent commit's only way: chunks of consecutive texts within the token budget (and the row cap), one mrk_encoder_embed
    each, then one mrk_index_build"""
    L = N.lib()
    before = timers(ctx)
    t = time.perf_counter()
    emb = np.empty((n, enc.dim), dtype=np.float32)
    lo = 0
    csum = np.concatenate([[0], np.cumsum(lens)])
    while lo < n:
        hi = int(np.searchsorted(csum, csum[lo] + budget, side="right")) - 1
        hi = min(max(hi, lo + 1), lo + ROW_CAP, n)
        N.check(L.mrk_encoder_embed(enc.handle, C.cast(C.byref(pt, lo * C.sizeof(C.c_char_p)), C.POINTER(C.c_char_p)), hi - lo, emb[lo:].ctypes.data))
        lo = hi
    h = C.c_void_p()
    N.check(L.mrk_index_build(ctx.handle, pi, emb.ctypes.data, 4, n, enc.dim, C.byref(h)))
    wall = time.perf_counter() - t
    after = timers(ctx)
    return HipIndex(h, ctx), wall, {k: after[k] - before[k] for k in after}


def summarise(walls, parts, n):
    w = np.array(walls)
    dev = np.array([p["encoder"] + p["knn_pool_pack"] + p["knn_norms"] for p in parts]) / 1e3
    return {"wall_s": [round(x, 4) for x in walls], "wall_s_median": float(np.median(w)), "items_per_s": float(n / np.median(w)),
            "spread": float((w.max() - w.min()) / np.median(w)), "encoder_ms": float(np.median([p["encoder"] for p in parts])),
            "pool_pack_ms": float(np.median([p["knn_pool_pack"] for p in parts])), "norms_ms": float(np.median([p["knn_norms"] for p in parts])),
            "device_idle_share": float(np.median(1.0 - dev / w))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--budget", type=int, default=0, help="max_tokens of the comparison (0: the library's default, 131 072)")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sorted", action="store_true")
    ap.add_argument("--catalogues", default="a,b")
    a = ap.parse_args()
    hip = Hip()
    ctx = M.Context(0)
    build = N.lib().mrk_build_id().decode()
    tok_json = synth.wordpiece_tokenizer_json(vocab_size=2000, max_length=MAX_LENGTH)
    free0 = hip.free_bytes()
    enc = HipEncoder(synth.bert_safetensors(synth.synthetic_bert(), 12), tok_json, ctx=ctx, precision="f32")
    ids = [f"item-{i}" for i in range(a.items)]
    pi, _ki = strs(ids)
    budget = a.budget or 131072
    for name in a.catalogues.split(","):
        texts, lens = catalogue(tok_json, a.items, 0.01 if name == "b" else 0.0)
        pt, _kt = strs(texts)
        tok = HipTokenizer(tok_json)
        t = time.perf_counter()
        for lo in range(0, a.items, 4096):
            tok.encode_batch(texts[lo:lo + 4096], capacity=MAX_LENGTH)
        tokenize_s = time.perf_counter() - t          # (includes this harness's marshalling of the strings: an upper bound)
        tok.close()
        head = {"catalogue": name, "items": a.items, "tokens": int(lens.sum()), "build": build, "host_tokenize_s_one_thread": tokenize_s}
        ctx.profile_enable(True)
        # warm-up of both forms (code objects, the scratch at its final size), and the check that they store the same bits
        x, _, _ = run_new(ctx, enc, pi, pt, a.items, budget)
        y, _, _ = run_parent(ctx, enc, pi, pt, a.items, lens, budget)
        sample = np.arange(0, a.items, max(a.items // 2000, 1))
        same = bool(np.array_equal(x.vectors(sample).view(np.uint64), y.vectors(sample).view(np.uint64)))
        table_bytes = x.info()["device_bytes"]
        x.close()
        y.close()
        held = free0 - hip.free_bytes()
        res = {"new": ([], []), "parent": ([], [])}
        for _ in range(a.rounds):
            for form in ("new", "parent"):
                ix, wall, parts = run_new(ctx, enc, pi, pt, a.items, budget) if form == "new" else run_parent(ctx, enc, pi, pt, a.items, lens, budget)
                ix.close()
                res[form][0].append(wall)
                res[form][1].append(parts)
        out = dict(head, case="new_vs_parent", max_tokens=budget, same_bits=same, index_bytes=table_bytes,
                   device_bytes_held_after_both_forms_without_an_index=held,
                   new=summarise(*res["new"], a.items), parent=summarise(*res["parent"], a.items))
        out["new_over_parent"] = out["new"]["wall_s_median"] / out["parent"]["wall_s_median"]
        print(json.dumps(out), flush=True)
        if a.sweep and name == "a":
            budgets = [8192, 32768, 65536, 131072]
            walls = {b: ([], []) for b in budgets}
            mem = {}
            for r in range(a.rounds + 1):               # round 0 warms every budget up (the scratch grows to the largest)
                for b in budgets:
                    before = hip.free_bytes()
                    ix, wall, parts = run_new(ctx, enc, pi, pt, a.items, b)
                    ix.close()
                    mem.setdefault(b, before - hip.free_bytes())
                    if r:
                        walls[b][0].append(wall)
                        walls[b][1].append(parts)
            H, I = enc.info["hidden"], enc.info["intermediate"]
            print(json.dumps(dict(head, case="max_tokens_sweep", scratch_bytes_per_token=H * 10 + 4 * H * 4 + I * 4,
                                  scratch_growth_first_call={str(b): mem[b] for b in budgets},
                                  sweep={str(b): summarise(*walls[b], a.items) for b in budgets})), flush=True)
        if a.sorted and name == "b":
            forms = {"input_order": "0", "sorted_windows": "4"}
            walls = {f: ([], []) for f in forms}
            for r in range(a.rounds + 1):
                for f, v in forms.items():
                    os.environ["MRK_SEMANTIC_WINDOW"] = v
                    N.reload_switches()
                    ix, wall, parts = run_new(ctx, enc, pi, pt, a.items, budget)
                    if r == 0 and f == "sorted_windows":
                        os.environ["MRK_SEMANTIC_WINDOW"] = "0"
                        N.reload_switches()
                        ref, _, _ = run_new(ctx, enc, pi, pt, a.items, budget)
                        same_sorted = bool(np.array_equal(ix.vectors(sample).view(np.uint64), ref.vectors(sample).view(np.uint64)))
                        ref.close()
                    ix.close()
                    if r:
                        walls[f][0].append(wall)
                        walls[f][1].append(parts)
            os.environ.pop("MRK_SEMANTIC_WINDOW")
            N.reload_switches()
            print(json.dumps(dict(head, case="length_sorted_windows", max_tokens=budget, same_bits=same_sorted,
                                  **{f: summarise(*walls[f], a.items) for f in forms})), flush=True)
        ctx.profile_enable(False)
    enc.close()
    ctx.close()


if __name__ == "__main__":
    main()
