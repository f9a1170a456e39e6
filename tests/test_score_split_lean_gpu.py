"""GPU: the split scorers after the round-17 trim (score_qs.hip: qs_score_byte_split_kernel, qs_score_split_kernel) against the
oracle, bit for bit.  What the trim changed and what can break with it:
 - the workgroup's LDS is [leaf values][exit leaves][slab]; the slab is read at an immediate offset (every NW, both leaf sizes;
   one forest wide enough that view * 256 + offset passes 64 KB);
 - the block that opens a ladder starts from the constant 0 and a block is one asm statement (forests whose nodes all sit in
   one ladder, stumps, chains);
 - whole chunks of 8 * NW trees run unrolled, the forest's last chunk in a loop (1, 7, 8 NW, 8 NW + 1, 2 * 8 NW + 3 trees);
 - the exit leaf's byte at both leaf sizes (8: LightGBM f64, 4: XGBoost f32 depth-4 complete trees, which also start from the
   base score), up to leaf 15 - the case a layout that stores the byte scaled by the leaf size would have to get right;
 - rows 1, 127, 128, 129, 257: tile edges and the `row < rows` guard.
One oracle prediction per forest, on the 257-row matrix; the shorter inputs are its leading rows (a row's score does not depend
on its batch)."""
import os

import numpy as np
import pytest

import metarank_amd as M
from oracle.forest import OracleForest
from workloads import synth

pytestmark = pytest.mark.gpu
NAN = float("nan")
KEYS = ("MRK_QS_BYTE", "MRK_QS_SPLIT", "MRK_QS_KERNEL", "MRK_SCORER", "MRK_QS_R", "MRK_WALK_TILE")
ROWS = (1, 127, 128, 129, 257)
COLS = 12
CAT_COL = 5
N_CATS = 40
BIG = 1.0e30


def tree_counts(nw):
    ch = 8 * nw
    return (1, 7, ch, ch + 1, 2 * ch + 3)


@pytest.fixture
def split_env():
    saved = {k: os.environ.get(k) for k in KEYS}
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    M.reload_switches()


def _predict(b, X, **env):
    for k in KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)
    M.reload_switches()
    return b.predict(X)


def make_X(seed, rows=ROWS[-1], cols=COLS, cat_col=CAT_COL):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(rows, cols))
    if cat_col is not None:
        X[:, cat_col] = rng.integers(-1, N_CATS + 2, size=rows)
    m = rng.random(X.shape)
    X[m < 0.05] = NAN
    X[(m >= 0.05) & (m < 0.1)] = 0.0
    return X


def quantiles_of(X, n=49):
    out = []
    for j in range(X.shape[1]):
        col = X[:, j][~np.isnan(X[:, j])]
        out.append(np.unique(np.quantile(col, np.linspace(0.001, 0.999, n))))
    return out


# ------------------------------------------------------------------------------------------- hand-shaped LightGBM trees
def lgbm_chain(rng, n_leaves, lean, thresholds, features):
    """A chain in LightGBM's numbering (the k-th split makes node k, keeps the split leaf on the left, leaf k + 1 on the right).
    lean="left": leaf 0 is split every time - every left subtree starts at position 0, and with <= 9 leaves all of them lie
    in positions 0-7 (the A ladder); lean="right": the newest leaf is split - the left subtrees are the single leaves
    0 .. n - 2, and a row that fails every test exits at the last position."""
    n = n_leaves - 1
    if lean == "left":
        left = [k + 1 for k in range(n - 1)] + [~0]
        right = [~(k + 1) for k in range(n)]
    else:
        left = [~k for k in range(n)]
        right = [k + 1 for k in range(n - 1)] + [~n]
    return {"num_leaves": n_leaves, "leaf_value": (rng.normal(size=n_leaves) * 0.01).tolist(),
            "split_feature": [int(f) for f in features[:n]], "threshold": [float(t) for t in thresholds[:n]],
            "decision_type": [int(rng.integers(3)) << 2 | (2 if rng.random() < 0.5 else 0) for _ in range(n)],
            "left_child": left, "right_child": right}


def numeric_features(rng, n):
    return [int(f) for f in rng.choice([c for c in range(COLS) if c != CAT_COL], size=n)]


def lgbm_master(X, n):
    """n trees, cycling through: random 16-leaf trees (some with categorical splits), short left chains (A ladder only),
    16-leaf right chains (both ladders, one node each), right chains no row passes a test of (exit leaf 15) and left chains
    every row passes every test of (exit leaf 0), small random trees."""
    rng = np.random.Generator(np.random.PCG64(11))
    q = quantiles_of(X)
    pick = lambda f: float(q[f][rng.integers(len(q[f]))])
    trees = []
    for i in range(n):
        kind = i % 7
        feats = numeric_features(rng, 15)
        if kind == 0:
            t = synth.random_lgbm_tree(rng, COLS, 16, 8, q, [CAT_COL], 0.15, N_CATS)
        elif kind == 1:
            t = lgbm_chain(rng, int(rng.integers(2, 10)), "left", [pick(f) for f in feats], feats)
        elif kind == 2:
            t = lgbm_chain(rng, 16, "right", [pick(f) for f in feats], feats)
        elif kind == 3:   # x <= -1e30 never holds (NaN: compared as 0.0, missing type None): every row ends at position 15
            t = lgbm_chain(rng, 16, "right", [-BIG] * 15, feats)
            t["decision_type"] = [0] * 15
        elif kind == 4:   # x <= 1e30 always holds: every row ends at position 0
            t = lgbm_chain(rng, 16, "left", [BIG] * 15, feats)
            t["decision_type"] = [0] * 15
        elif kind == 5:
            t = synth.random_lgbm_tree(rng, COLS, int(rng.integers(1, 16)), 8, q)
        else:
            t = synth.random_lgbm_tree(rng, COLS, 16, 4, q)   # balanced: nodes in both ladders and across them
        trees.append(t)
    return trees


def xgb_master(X, n):
    """depth-4 complete trees (16 f32 leaves); every seventh tree sends every row to leaf 15 (x < -1e30 never holds), every
    seventh one to leaf 0; some categorical splits."""
    rng = np.random.Generator(np.random.PCG64(12))
    q = quantiles_of(X)
    trees = []
    for i in range(n):
        kind = i % 7
        cat = (kind == 0)
        t = synth.random_xgb_tree(rng, COLS, 4, q, [CAT_COL] if cat else None, 0.2 if cat else 0.0, N_CATS, True)
        if kind in (3, 4):
            internal = [j for j, l in enumerate(t["left_children"]) if l >= 0]
            for j in internal:
                t["split_conditions"][j] = -BIG if kind == 3 else BIG
                t["default_left"][j] = 0 if kind == 3 else 1   # NaN follows the other rows
        trees.append(t)
    return trees


@pytest.fixture(scope="module")
def forests():
    """backend -> (X, {n_trees: (model blob, oracle scores of X)}) for every tree count any NW asks for"""
    X = make_X(1)
    counts = sorted({n for nw in (2, 4, 8, 16) for n in tree_counts(nw)})
    lg, xg = lgbm_master(X, counts[-1]), xgb_master(X, counts[-1])
    out = {"lightgbm": (X, {}), "xgboost": (X, {})}
    for n in counts:
        blob = synth.write_lightgbm_text(lg[:n], COLS)
        out["lightgbm"][1][n] = (blob, OracleForest.from_lightgbm_text(blob).predict(X))
        blob = synth.write_xgboost_json(synth.xgboost_document([dict(t) for t in xg[:n]], COLS, 0.5))
        out["xgboost"][1][n] = (blob, OracleForest.from_xgboost(blob).predict(X))
    return out


def test_the_forests_reach_the_extremes():
    """(the oracle alone) the hand-shaped trees do what the cases below need them for: every row leaves tree 3 at its last
    position, 15, and tree 4 at position 0"""
    X = make_X(1)
    lg, xg = lgbm_master(X, 7), xgb_master(X, 7)
    for k, leaf in ((3, 15), (4, 0)):
        assert lg[k]["num_leaves"] == 16
        got = OracleForest.from_lightgbm_text(synth.write_lightgbm_text([lg[k]], COLS)).predict(X)
        assert np.array_equal(got, np.full(len(X), lg[k]["leaf_value"][leaf]))
        t = xg[k]
        leaves = [j for j, l in enumerate(t["left_children"]) if l < 0]   # BFS numbering: left to right
        assert len(leaves) == 16
        got = OracleForest.from_xgboost(synth.write_xgboost_json(synth.xgboost_document([dict(t)], COLS, 0.5))).predict(X)
        want = np.float32(0.5) + np.float32(t["split_conditions"][leaves[leaf]])
        assert np.array_equal(got, np.full(len(X), float(want)))


@pytest.mark.parametrize("nw", [2, 4, 8, 16])
@pytest.mark.parametrize("backend", ["lightgbm", "xgboost"])
def test_split_kernels_match_the_oracle(split_env, forests, backend, nw):
    X, by_n = forests[backend]
    ctx = M.default_context()
    for n in tree_counts(nw):
        blob, exp = by_n[n]
        b = M.HipBooster(blob, M.LIGHTGBM if backend == "lightgbm" else M.XGBOOST, ctx)
        try:
            assert b.info()["bitvector"] == 1 and b.info()["n_trees"] == n and b.info()["is_f64"] == (backend == "lightgbm")
            for byte in (None, "0"):     # byte-mode kernel / the 16-bit split kernel
                env = {"MRK_QS_KERNEL": "1", "MRK_QS_SPLIT": str(nw)}
                if byte is not None:
                    env["MRK_QS_BYTE"] = byte
                for rows in ROWS:
                    got = _predict(b, X[:rows], **env)
                    assert got.shape == (rows,)
                    assert np.array_equal(got, exp[:rows]), f"{backend}, {n} trees, NW {nw}, MRK_QS_BYTE={byte}, {rows} rows"
        finally:
            b.close()


@pytest.mark.parametrize("nw", [2, 4, 8, 16])
def test_single_ladder_forests(split_env, nw):
    """every tree a short left chain (all nodes A-only: the B ladder's masks are zero) / every tree a 2-leaf stump; and every
    tree a 16-leaf right chain (8 A-only and 7 B-only nodes, no crossing one)"""
    X = make_X(2, cat_col=None)
    q = quantiles_of(X)
    rng = np.random.Generator(np.random.PCG64(13))
    n = 8 * nw + 1
    ctx = M.default_context()
    for shape in ("left9", "stump", "right16"):
        trees = []
        for _ in range(n):
            feats = [int(f) for f in rng.integers(COLS, size=15)]
            thr = [float(q[f][rng.integers(len(q[f]))]) for f in feats]
            trees.append(lgbm_chain(rng, {"left9": 9, "stump": 2, "right16": 16}[shape], "right" if shape == "right16" else "left", thr, feats))
        blob = synth.write_lightgbm_text(trees, COLS)
        exp = OracleForest.from_lightgbm_text(blob).predict(X)
        b = M.HipBooster(blob, M.LIGHTGBM, ctx)
        try:
            for byte in ({}, {"MRK_QS_BYTE": "0"}):
                got = _predict(b, X, MRK_QS_KERNEL="1", MRK_QS_SPLIT=str(nw), **byte)
                assert np.array_equal(got, exp), f"{shape}, NW {nw}, {byte}"
        finally:
            b.close()


@pytest.mark.parametrize("nw", [2, 4, 8, 16])
def test_categorical_forest(split_env, nw):
    """categorical nodes read the unclamped cells: the byte kernel from the global tile, the 16-bit kernel from the moved slab"""
    X = make_X(3)
    n = 2 * 8 * nw + 3
    blob = synth.synthetic_lgbm_model(n_trees=n, n_features=COLS, quantiles=quantiles_of(X), cat_features=[CAT_COL], cat_prob=0.3,
                                      n_cats=N_CATS, seed=nw)
    exp = OracleForest.from_lightgbm_text(blob).predict(X)
    xb = synth.synthetic_xgb_model(n_trees=n, n_features=COLS, depth=4, quantiles=quantiles_of(X), cat_features=[CAT_COL], cat_prob=0.3,
                                   n_cats=N_CATS, seed=nw)
    expx = OracleForest.from_xgboost(xb).predict(X)
    ctx = M.default_context()
    for blob_, kind, want in ((blob, M.LIGHTGBM, exp), (xb, M.XGBOOST, expx)):
        b = M.HipBooster(blob_, kind, ctx)
        try:
            assert b.info()["n_categorical"] > 0
            for byte in ({}, {"MRK_QS_BYTE": "0"}):
                for rows in (129, 257):
                    got = _predict(b, X[:rows], MRK_QS_KERNEL="1", MRK_QS_SPLIT=str(nw), **byte)
                    assert np.array_equal(got, want[:rows]), f"backend {kind}, NW {nw}, {byte}, {rows} rows"
        finally:
            b.close()


@pytest.mark.parametrize("nw", [2, 4, 8, 16])
def test_threshold_table_longer_than_254(split_env, nw):
    """300 distinct thresholds on column 0 (20 right chains of 15 nodes): k passes 254, byte mode is refused, and the 16-bit
    split kernel - same layout - scores the forest"""
    rng = np.random.Generator(np.random.PCG64(14))
    X = make_X(4, cat_col=None)
    thr = np.sort(rng.normal(size=300))
    trees = [lgbm_chain(rng, 16, "right", rng.permutation(thr[15 * i:15 * i + 15]), [0] * 15) for i in range(20)]
    q = quantiles_of(X)
    while len(trees) < 8 * nw + 1:
        trees.append(synth.random_lgbm_tree(rng, COLS, 16, 8, q))
    blob = synth.write_lightgbm_text(trees, COLS)
    exp = OracleForest.from_lightgbm_text(blob).predict(X)
    b = M.HipBooster(blob, M.LIGHTGBM, M.default_context())
    try:
        for rows in (128, 257):
            assert np.array_equal(_predict(b, X[:rows], MRK_QS_KERNEL="1", MRK_QS_SPLIT=str(nw)), exp[:rows]), f"NW {nw}, {rows} rows"
    finally:
        b.close()


def test_slab_offset_plus_view_passes_64k(split_env):
    """130 columns (about 210 views: a view is a column under one missing rule), 16 wavefronts, f64 leaves: the slab starts at
    byte 32 768 and its views from the 128th on lie beyond byte 65 536 - the add-TID read's address is M0 + offset + 4 * lane
    with no 16-bit wrap"""
    X = make_X(5, rows=129, cols=130, cat_col=None)
    blob = synth.synthetic_lgbm_model(n_trees=8 * 16 + 1, n_features=130, quantiles=quantiles_of(X, 9), missing="per_feature", seed=5)
    exp = OracleForest.from_lightgbm_text(blob).predict(X)
    b = M.HipBooster(blob, M.LIGHTGBM, M.default_context())
    try:
        assert b.info()["tile_columns"] > 160
        for byte in ({}, {"MRK_QS_BYTE": "0"}):
            for nw in ("16", "8"):
                assert np.array_equal(_predict(b, X, MRK_QS_KERNEL="1", MRK_QS_SPLIT=nw, **byte), exp), f"NW {nw}, {byte}"
    finally:
        b.close()
