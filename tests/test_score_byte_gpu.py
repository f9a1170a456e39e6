"""GPU: the bit-vector scorer's byte mode (score_qs.hip qs_score_byte_split_kernel: forests whose numerical nodes all have
k <= 254, cells clamped to 255, one v_pk_sub_i16 per node) against the 16-bit kernels (MRK_QS_BYTE=0) and the oracle, bit for
bit: 16-leaf and smaller trees, per-node missing rules, categorical nodes, columns of 255 thresholds (k = 254) and of more
(byte mode refused), every split width, c2- and c3-shaped inputs.  The host-side image and step are emulated exhaustively by
tests/test_qs_byte_cpu.py."""
import os

import numpy as np
import pytest

import metarank_amd as M
from oracle.forest import OracleForest
from workloads import synth

pytestmark = pytest.mark.gpu
NAN = float("nan")
KEYS = ("MRK_QS_BYTE", "MRK_QS_SPLIT", "MRK_QS_KERNEL", "MRK_SCORER")


@pytest.fixture
def byte_env():
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


def make_X(rng, rows, cols, cat_col=None, n_cats=40):
    X = rng.normal(size=(rows, cols))
    if cat_col is not None:
        X[:, cat_col] = rng.integers(-1, n_cats + 2, size=rows)
    m = rng.random(X.shape)
    X[m < 0.05] = NAN
    X[(m >= 0.05) & (m < 0.1)] = 0.0
    return X


def quantiles_of(X, n):
    out = []
    for j in range(X.shape[1]):
        col = X[:, j][~np.isnan(X[:, j])]
        out.append(np.unique(np.quantile(col, np.linspace(0.001, 0.999, n))))
    return out


def check(blob, X, splits=("2", "4", "8", "16", None)):
    exp = OracleForest.from_lightgbm_text(blob).predict(X)
    ctx = M.default_context()
    b = M.HipBooster(blob, M.LIGHTGBM, ctx)
    try:
        for nw in splits:
            env = {} if nw is None else {"MRK_QS_SPLIT": nw}
            byte = _predict(b, X, **env)
            old = _predict(b, X, MRK_QS_BYTE="0", **env)
            assert np.array_equal(byte, old), f"split {nw}: byte mode differs from the 16-bit kernel"
            assert np.array_equal(byte, exp), f"split {nw}: differs from the oracle"
    finally:
        b.close()


@pytest.mark.parametrize("num_leaves,missing,cat_prob", [(16, "per_node", 0.05), (16, "per_feature", 0.0), (7, "per_node", 0.1),
                                                         (2, "per_feature", 0.3)])
def test_byte_mode_matches_16_bit_kernels(byte_env, num_leaves, missing, cat_prob):
    rng = np.random.default_rng(num_leaves * 7 + len(missing))
    X = make_X(rng, 1000, 24, cat_col=7)
    blob = synth.synthetic_lgbm_model(n_trees=200, n_features=24, num_leaves=num_leaves, quantiles=quantiles_of(X, 49),
                                      cat_features=[7], cat_prob=cat_prob, n_cats=40, missing=missing, seed=num_leaves)
    check(blob, X)


@pytest.mark.parametrize("n_thr", [255, 254, 300])
def test_byte_mode_threshold_table_limits(byte_env, n_thr):
    """255 thresholds per column: k up to 254, byte mode; 300: refused, the 16-bit kernel scores it"""
    rng = np.random.default_rng(n_thr)
    X = make_X(rng, 2000, 12)
    n_trees = 1000 if n_thr > 255 else 300  # (enough nodes to use more than 255 of 300 candidates on a column)
    blob = synth.synthetic_lgbm_model(n_trees=n_trees, n_features=12, quantiles=quantiles_of(X, n_thr), missing="per_node", seed=n_thr)
    check(blob, X)


@pytest.mark.parametrize("rows,cols", [(38400, 24), (20000, 64)])
def test_byte_mode_c2_c3_shapes(byte_env, rows, cols):
    """c2: the benchmark's forest (500 16-leaf trees, 49 quantiles per column, ~1 categorical split per 10 trees); c3: 64 columns"""
    rng = np.random.default_rng(rows)
    X = make_X(rng, rows, cols, cat_col=7)
    blob = synth.synthetic_lgbm_model(n_trees=500, n_features=cols, quantiles=quantiles_of(X[:4000], 49), cat_features=[7],
                                      cat_prob=0.007, missing="per_feature")
    check(blob, X, splits=("4", "8", None))
