"""Launch shapes chosen from a batch's shape (metarank_amd/csrc/launch_shape.hpp): host arithmetic, no device.

Each expectation is the choice an A/B measurement on the MI355X ended in (profiles/r02_r_slices.txt,
profiles/r02_ab_runs.json, gpurun_out/r02_l); the test keeps a later edit of the rules from silently moving the
BASELINE configurations onto a shape that was measured slower."""
import ctypes as C

import pytest

from metarank_amd import _native


@pytest.fixture(scope="module")
def lib():
    L = _native.lib()
    L.mrk_debug_fused_shape.restype = C.c_int
    L.mrk_debug_fused_shape.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.mrk_debug_scorer_split.restype = C.c_int
    L.mrk_debug_scorer_split.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    return L


def fused(lib, n_req, max_items):
    out = (C.c_int * 3)()
    assert lib.mrk_debug_fused_shape(n_req, max_items, out) == 0
    return tuple(out)  # (lanes per workgroup, op split, slices per request)


@pytest.mark.parametrize("n_req,max_items,want,why", [
    (3840, 100, (128, 1, 1), "c2: two wavefronts per request (64 lanes = two serial rounds: 0.421 vs 0.288 ms)"),
    (384, 1000, (256, 1, 2), "c3: two workgroups per request fill one residency (0.62 -> 0.43 ms; 3 / 4 slices: 0.47 / 0.48)"),
    (96, 1000, (256, 1, 4), "96 large requests: one workgroup per round of the lanes (0.52 -> 0.21 ms)"),
    (1, 100, (512, 4, 1), "a single /rank request: four copies of the item lanes share the ops (p50 0.19 -> 0.158 ms)"),
    (16, 100, (512, 4, 1), "... up to 16 requests"),
    (64, 100, (512, 4, 1), "... and up to 64 when they are small (mrk_rank's combined batches: 188 k -> 228 k requests/s at 64 callers, r06_x)"),
    (65, 100, (128, 1, 1), "... and not beyond"),
    (17, 1000, (256, 1, 4), "17 large requests keep their slices"),
    (1, 1000, (512, 2, 1), "a single 1 000-item request: 256 item lanes leave room for two copies; no slices on top of a split"),
    (1, 1, (256, 4, 1), "one candidate: one wavefront of item lanes, four copies"),
    (3840, 300, (256, 1, 1), "a full batch of 300-item requests: 2 rounds, but 3 840 x 4 wavefronts already exceed a residency"),
    (4096, 64, (64, 1, 1), "64-item requests: one wavefront each"),
])
def test_fused_kernel_shape(lib, n_req, max_items, want, why):
    assert fused(lib, n_req, max_items) == want, why


def test_slices_never_exceed_the_rounds_or_one_residency(lib):
    for n_req in (17, 32, 100, 384, 1000, 5000):
        for items in (65, 128, 257, 512, 700, 1000, 1024):
            lanes, split, slices = fused(lib, n_req, items)
            rounds = -(-items // (lanes // split))
            assert 1 <= slices <= rounds
            assert slices == 1 or n_req * (lanes // 64) * slices <= 4096


@pytest.mark.parametrize("rows,views,f64,want,why", [
    (384_000, 41, 1, 4, "c2 (V = 41): 1 -> 0.283 ms, 2 -> 0.317, 4 -> 0.218, 8 -> 0.220, 16 -> 0.230"),
    (384_000, 100, 1, 8, "c3-like (V ~ 100): 1 -> 0.547 ms, 4 -> 0.280, 8 -> 0.248"),
    (100, 41, 1, 16, "a single request: one tile, every wavefront the kernel has"),
    (100_000, 41, 1, 8, "c4: 782 tiles (r04_h: 4 -> 0.098 ms, 8 -> 0.083, 16 -> 0.083)"),
    (20_000, 41, 1, 16, "157 tiles (r04_h: 4 -> 0.066 ms, 8 -> 0.045, 16 -> 0.032)"),
    (400_000, 41, 1, 4, "3 125 tiles (r04_h: 4 -> 0.231 ms, 8 -> 0.233, 16 -> 0.242)"),
    (4_000_000, 41, 1, 4, "c4x: 31 250 tiles"),
    (384_000, 0, 1, 1, "a forest of single-leaf trees has no views (and no division by zero: r02_m)"),
])
def test_scorer_wavefronts_per_tile(lib, rows, views, f64, want, why):
    assert lib.mrk_debug_scorer_split(rows, views, f64, 256) == want, why


# ---- which pipeline a batch runs (metarank_amd/csrc/rank_plan.hpp), under the default switches
ONE, ONE_WALK, FUSED_CELLS, ITEM_CELLS, MATRIX = range(5)                       # RankPath
JIT_RANK, JIT_SPLIT, JIT_MATRIX, JIT_ITEMS, JIT_ONE, JIT_ONE_WALK, JIT_VALUES, JIT_NONE = 0, 1, 2, 3, 4, 9, 11, -2
PLAN_INPUTS = ["n_req", "items", "entries", "doubles", "compact", "overrides", "want_matrix", "normalises", "n_prep", "dim",
               "model", "bitvector", "f64", "thr_cap", "n_views", "rt_doubles", "chunk_bytes", "chunk_trees",
               "lo", "hi", "sort", "direct", "rank_one_walk", "scorer_walk"]
# a bit-vector LightGBM model over the stock Ranklens program (24 columns, 9 pre-pass reductions, 41 views, 740 resident thresholds),
# tables that fit a workgroup's LDS and the compact entry, no overrides, no matrix asked for, the whole range, sort on
PLAN_DEFAULTS = dict(n_req=1, items=100, entries=1024, doubles=100, compact=1, overrides=0, want_matrix=0, normalises=0, n_prep=9, dim=24,
                     model=1, bitvector=1, f64=1, thr_cap=128, n_views=41, rt_doubles=740, chunk_bytes=0, chunk_trees=0,
                     lo=0, hi=-1, sort=1, direct=0, rank_one_walk=-1, scorer_walk=0)
# a forest of 64-leaf trees: no bit-vector image; the tree-walk image's largest chunk is 24 KB of 65 trees
DEEP = dict(bitvector=0, thr_cap=0, n_views=0, rt_doubles=0, chunk_bytes=24 * 1024, chunk_trees=65)


def plan(values=0, **kw):
    L = _native.lib()
    L.mrk_debug_rank_plan.restype = C.c_int
    L.mrk_debug_rank_plan.argtypes = [C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64)]
    assert not set(kw) - set(PLAN_INPUTS), kw
    args = dict(PLAN_DEFAULTS, **kw)
    inp = (C.c_int64 * len(PLAN_INPUTS))(*[args[k] for k in PLAN_INPUTS])
    out = (C.c_int64 * 8)()
    assert L.mrk_debug_rank_plan(inp, values, out) == 0
    if values:
        return dict(one=int(out[0]), kernel=int(out[1]))
    return dict(zip(("path", "kernel", "items_rt", "prepass", "keyed", "whole_matrix", "entry_bytes", "split_kernel"), (int(x) for x in out)))


@pytest.mark.parametrize("shape,want,why", [
    (dict(n_req=3840, items=100), dict(path=FUSED_CELLS, kernel=JIT_RANK, entry_bytes=4, split_kernel=0, keyed=1), "c2: the plain kernel, compact tables, keyed by the forest"),
    (dict(n_req=3840, items=100, compact=0), dict(path=FUSED_CELLS, kernel=JIT_SPLIT, entry_bytes=8, split_kernel=1, keyed=1), "a table the 4-byte entries do not hold: the split kernel at op split 1"),
    (dict(n_req=384, items=1000), dict(path=FUSED_CELLS, kernel=JIT_SPLIT, entry_bytes=8, split_kernel=1), "c3: two slices"),
    (dict(n_req=1, items=100_000), dict(path=ITEM_CELLS, kernel=JIT_ITEMS, items_rt=1, prepass=1, keyed=1), "c4: pre-pass + item-parallel assembly"),
    (dict(n_req=1, items=100_000, n_prep=0), dict(path=ITEM_CELLS, kernel=JIT_ITEMS, items_rt=1, prepass=0), "... no pre-pass kernel for a program without reductions"),
    (dict(direct=1), dict(path=ONE, kernel=JIT_ONE, keyed=1), "mrk_rank, one request of 100 candidates: one launch"),
    (dict(direct=1, items=128), dict(path=ONE, kernel=JIT_ONE), "... up to a scorer tile of candidates"),
    (dict(direct=1, items=129), dict(path=FUSED_CELLS, kernel=JIT_SPLIT), "... and not one more"),
    (dict(direct=1, n_req=128), dict(path=ONE, kernel=JIT_ONE), "the front's combined batches: up to MRK_RANK_ONE_MAX = 128 requests"),
    (dict(direct=1, n_req=129), dict(path=FUSED_CELLS, kernel=JIT_RANK, entry_bytes=4), "... and not one more"),
    (dict(direct=1, n_req=2, lo=128), dict(path=FUSED_CELLS, kernel=JIT_SPLIT), "a slice of the batch is never one launch"),
    (dict(direct=1, sort=0), dict(path=FUSED_CELLS, kernel=JIT_SPLIT), "... nor a run that does not order"),
    (dict(direct=1, overrides=1), dict(path=FUSED_CELLS, kernel=JIT_SPLIT), "... nor a request with per-item overrides"),
    (dict(direct=0), dict(path=FUSED_CELLS, kernel=JIT_SPLIT, split_kernel=1), "a prepared batch of one request: its caller reads device memory"),
    (dict(want_matrix=1), dict(path=MATRIX, kernel=JIT_NONE), "explain: the matrix kernel has no op-split form (op split 4 here)"),
    (dict(want_matrix=1, direct=1), dict(path=MATRIX, kernel=JIT_NONE), "... through mrk_rank too"),
    (dict(want_matrix=1, n_req=3840), dict(path=MATRIX, kernel=JIT_MATRIX, keyed=0), "... a full batch takes the specialised matrix kernel"),
    (dict(normalises=1, n_req=3840, hi=3840 * 50), dict(path=MATRIX, kernel=JIT_MATRIX, whole_matrix=1), "a shard of a normalising program assembles the whole batch"),
    (dict(normalises=1, n_req=3840), dict(path=MATRIX, kernel=JIT_MATRIX, whole_matrix=0), "... the whole range is not a shard"),
    (dict(model=0, n_req=3840), dict(path=MATRIX, kernel=JIT_NONE), "no model (NoopRanker): the interpreting matrix kernel"),
    (dict(direct=1, **DEEP), dict(path=MATRIX, kernel=JIT_NONE), "a forest without a bit-vector image: mrk_rank keeps its three launches"),
    (dict(direct=1, rank_one_walk=1, **DEEP), dict(path=ONE_WALK, kernel=JIT_ONE_WALK, keyed=0), "... unless MRK_RANK_ONE_WALK=1"),
    (dict(direct=1, rank_one_walk=1, want_matrix=1, **DEEP), dict(path=MATRIX, kernel=JIT_NONE), "... and not with the matrix asked for"),
    (dict(direct=1, rank_one_walk=1, dim=64, **DEEP), dict(path=MATRIX, kernel=JIT_NONE), "... nor when matrix and chunk pass 96 KB of LDS"),
    (dict(n_req=3840, scorer_walk=1), dict(path=MATRIX, kernel=JIT_MATRIX), "MRK_SCORER=walk on a bit-vector model"),
    (dict(direct=1, scorer_walk=1), dict(path=MATRIX, kernel=JIT_NONE), "... for mrk_rank too (MRK_RANK_ONE_WALK unset)"),
    (dict(items=0), dict(path=MATRIX), "a request without candidates"),
    (dict(n_req=0, items=0), dict(path=MATRIX, kernel=JIT_NONE), "an empty batch"),
])
def test_rank_plan(shape, want, why):
    got = plan(**shape)
    assert {k: got[k] for k in want} == want, (why, got)


@pytest.mark.parametrize("shape,want,why", [
    (dict(), dict(one=1, kernel=JIT_VALUES), "mrk_values: one launch into pinned memory"),
    (dict(n_req=384, items=1000), dict(one=0, kernel=JIT_NONE), "sliced requests: the matrix path, interpreting"),
    (dict(n_req=3840, want_matrix=1), dict(one=0, kernel=JIT_MATRIX), "the device matrix asked for: the matrix path, its specialised kernel on a plain shape"),
    (dict(overrides=1), dict(one=0, kernel=JIT_NONE), "per-item overrides"),
])
def test_values_plan(shape, want, why):
    assert plan(values=1, **shape) == want, why
