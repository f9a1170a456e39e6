"""Decodable forests over exactly known threshold tables, probe rows one ulp either side of every threshold, and a numpy
reference of the two libraries' decision rules (shared by test_boundary_bins_cpu.py and test_boundary_bins_gpu.py).

Every forest score hangs on one integer per (row, column): bin(x) = #{t in T_col : t < x} for LightGBM, #{t : t <= x}
after the f64 -> f32 narrowing for XGBoost.  The forests built here make that integer readable from the score: a column's
sorted table is cut into runs of at most 15 consecutive thresholds, each run is one balanced search tree whose leaves,
left to right, hold 0, 1, 2, ... - a row's exit leaf is its bin within the run, so the column's trees add up to bin(x)
and every score is a small integer (exact in f64 and f32).  A 15-threshold run is a full 16-leaf tree.

Nothing here reads model bytes or the oracle: `reference_scores` walks the tree descriptions of this module,
`searchsorted_bins` counts with numpy.
"""
from __future__ import annotations

from collections import deque

import numpy as np

from workloads import synth

SEED = 20261017
KZERO = float(np.float32(1e-35))              # LightGBM kZeroThreshold, (double)1e-35f
DBL_MAX = float(np.finfo(np.float64).max)     # 1.7976931348623157e308
FLT_MAX = float(np.finfo(np.float32).max)
FLT_DENORM = float(np.float32(1e-45))         # the smallest f32 denormal, 2^-149
INF, NAN = float("inf"), float("nan")
RUN = 15                                      # thresholds per tree: at most 16 leaves (the bit-vector scorer's limit)

# (missing type, default left) of a tree's nodes.  LightGBM: decision_type bits 2-3 = None 0 / Zero 1 / NaN 2
LGBM_RULES = [(0, False), (1, True), (1, False), (2, True), (2, False)]
XGB_RULES = [(2, True), (2, False)]           # NaN is "missing": default left / default right

# table lengths per split-on column; "U": a column the forest never splits on.  One more matrix column follows the last
# (beyond the forest's num_feature).  XGBoost forests get one more split-on column (XGB_EXTRA), so that the number of
# split-on columns mod 4 - the shapes of the resident-table sink's last group - takes 0, 1, 2 and 3 over the layouts.
LAYOUTS = {
    # resident everywhere: 499 doubles                                                    (24 | 25 split-on columns)
    "S": [1, 2, 3, 4, 5, "U", 7, 8, 9, 15, 16, 17, 31, "U", 32, 33, 63, 64, 65, 1, 2, 3, 5, 16, 33, 64],
    # chunk and byte edges: 2097 doubles = 16.4 KB: staged by the fused kernel, resident in the split kernel; k up to 254
    "M": [1, 2, 127, 3, 4, "U", 128, 5, 7, 129, 8, 9, 191, 15, 16, 192, "U", 17, 31, 193, 32, 33, 253, 63, 64, 254, 65, 255],  # 26 | 27
    # beyond byte mode and beyond the staged / resident limit: long tables next to short ones
    "L": [1, 256, 2, 4, 257, "U", 8, 15, 300, 16, 127, 128, 17, 520, 129, 33, 191, "U", 192, 64, 193, 253, 65, 254, 255],   # 23 | 24
}
XGB_EXTRA = 9
ALL_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 253, 254, 255, 256, 257, 300]
ZERO_CLUSTER_LENGTHS = (7, 9, 16, 33, 65, 129, 192, 255, 257)   # tables that hold the zero-flush cluster


def f32(x) -> float:
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def next_f32(x: float, up: bool) -> float:
    with np.errstate(over="ignore"):
        return float(np.nextafter(np.float32(x), np.float32(INF if up else -INF)))


def next_f64(x: float, up: bool) -> float:
    with np.errstate(over="ignore"):
        return float(np.nextafter(x, INF if up else -INF))


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Tree:
    """One balanced search tree over `thr` (sorted) on column `col`: nodes[i] = (threshold, left, right), a child >= 0 is
    a node, ~child a leaf; leaves are numbered left to right and leaf j has value j."""

    def __init__(self, col, thr, rule):
        self.col, self.thr, self.rule = col, list(thr), rule
        self.nodes = []
        self._build(0, len(self.thr))
        self.n_leaves = len(self.thr) + 1

    def _build(self, lo, hi) -> int:
        if lo == hi:
            return ~lo
        mid = (lo + hi) // 2
        k = len(self.nodes)
        self.nodes.append(None)
        left = self._build(lo, mid)
        right = self._build(mid + 1, hi)
        self.nodes[k] = (self.thr[mid], left, right)
        return k


class BoundaryForest:
    def __init__(self, layout: str, backend: str, rules: str = "per_feature", seed: int = SEED):
        assert backend in ("lgbm", "xgb") and rules in ("per_feature", "per_tree")
        self.layout, self.backend, self.is_xgb = layout, backend, backend == "xgb"
        rng = np.random.Generator(np.random.PCG64([seed, sum(map(ord, layout)), int(self.is_xgb)]))
        lengths = list(LAYOUTS[layout]) + ([XGB_EXTRA] if self.is_xgb else [])
        self.num_feature = len(lengths)
        self.n_cols = self.num_feature + 1        # one matrix column beyond the forest's num_feature
        self.split_cols = [c for c, n in enumerate(lengths) if n != "U"]
        self.unsplit_cols = [c for c, n in enumerate(lengths) if n == "U"] + [self.num_feature]
        self.lengths = {c: lengths[c] for c in self.split_cols}
        self.tables = {c: self._table(rng, c, lengths[c]) for c in self.split_cols}   # node thresholds, sorted
        all_rules = XGB_RULES if self.is_xgb else LGBM_RULES
        self.trees = []
        for k, c in enumerate(self.split_cols):
            T = self.tables[c]
            for lo in range(0, len(T), RUN):
                rule = all_rules[k % len(all_rules)] if rules == "per_feature" else all_rules[int(rng.integers(len(all_rules)))]
                self.trees.append(Tree(c, T[lo:lo + RUN], rule))
        # below every table and not missing (LightGBM: -inf is an ordinary value; XGBoost rejects it, no table reaches -FLT_MAX)
        self.neutral = -FLT_MAX if self.is_xgb else -INF
        self.above = FLT_MAX if self.is_xgb else INF

    # ---- tables
    def _table(self, rng, col, n) -> np.ndarray:
        """`n` distinct, strictly increasing thresholds; the node list may carry one more entry: -0.0 next to 0.0"""
        x = self.is_xgb
        r = (lambda v: f32(v)) if x else (lambda v: v)
        special = []
        if n == 1:
            special = [0.0]
        elif n == 2:
            special = [FLT_DENORM, FLT_MAX] if x else [-DBL_MAX, DBL_MAX]
        elif n in ZERO_CLUSTER_LENGTHS:
            special = [0.0] + [s * r(v) for v in (1e-36, 1e-37, KZERO) for s in (1.0, -1.0)]
        if n in (128, 255, 256, 300, 520, 64):    # extremes at the ends of chunk-, byte- and limit-sized tables
            special += [FLT_MAX, -FLT_DENORM, FLT_DENORM] if x else [-DBL_MAX, DBL_MAX]
        if n in (4, 15, 31, 63, 127, 191, 253, 254) or n >= 256:   # two adjacent representable values
            a = r(float(rng.normal() * 3))
            special += [a, next_f32(a, True) if x else next_f64(a, True)]
        vals = set(special)
        assert len(vals) == len(special) <= n, (n, special)
        while len(vals) < n:
            v = r(float(rng.normal() * (10.0 ** int(rng.integers(-2, 4)))))
            if v != 0.0 and abs(v) > 1e-30:
                vals.add(v)
        T = sorted(vals)
        if 0.0 in vals and n in (9, 33, 129, 257):   # -0.0 and 0.0 in different nodes of the column: the packer merges them
            T.insert(T.index(0.0), -0.0)
        T = np.array(T, dtype=np.float64)
        assert (T[1:] >= T[:-1]).all() and len(np.unique(T)) == n
        return T

    # ---- model files, through the project's own writers
    def model_bytes(self) -> bytes:
        if self.is_xgb:
            return synth.write_xgboost_json(synth.xgboost_document([self._xgb_tree(t) for t in self.trees], self.num_feature, 0.5))
        return synth.write_lightgbm_text([self._lgbm_tree(t) for t in self.trees], self.num_feature)

    @staticmethod
    def _lgbm_tree(t: Tree) -> dict:
        """LightGBM's node numbering (Tree::Split, as workloads/synth.random_lgbm_tree): the k-th split creates internal node
        k, the split leaf keeps its index on the left, the right child becomes leaf k + 1"""
        mt, dl = t.rule
        n = len(t.thr)
        feat, thr, dt, left, right = [], [], [], [], []
        leaf_value = [0.0] * (n + 1)
        todo = deque([(0, n, 0, -1, 0)])          # (lo, hi, leaf id, parent, side)
        while todo:
            lo, hi, leaf, parent, side = todo.popleft()
            if lo == hi:
                leaf_value[leaf] = float(lo)
                continue
            k = len(feat)
            if parent >= 0:
                (left if side == 0 else right)[parent] = k
            mid = (lo + hi) // 2
            feat.append(t.col)
            thr.append(float(t.thr[mid]))
            dt.append((2 if dl else 0) | (mt << 2))
            left.append(~leaf)
            right.append(~(k + 1))
            todo.append((lo, mid, leaf, k, 0))
            todo.append((mid + 1, hi, k + 1, k, 1))
        return {"num_leaves": n + 1, "leaf_value": leaf_value, "split_feature": feat, "threshold": thr, "decision_type": dt,
                "left_child": left, "right_child": right}

    def _xgb_tree(self, t: Tree) -> dict:
        """gbtree RegTree arrays, nodes numbered breadth-first; a leaf's value is its split_condition"""
        _, dl = t.rule
        recs = {}
        todo = deque([(0, len(t.thr), 0, 2147483647)])
        next_id = 1
        while todo:
            lo, hi, nid, par = todo.popleft()
            if lo == hi:
                recs[nid] = (-1, -1, par, 0, float(lo), 0)
                continue
            mid = (lo + hi) // 2
            l, r = next_id, next_id + 1
            next_id += 2
            recs[nid] = (l, r, par, t.col, float(t.thr[mid]), int(dl))
            todo.append((lo, mid, l, nid))
            todo.append((mid + 1, hi, r, nid))
        n = next_id
        col = lambda i: [recs[k][i] for k in range(n)]
        return {"base_weights": [0.0] * n, "categories": [], "categories_nodes": [], "categories_segments": [], "categories_sizes": [],
                "default_left": col(5), "id": 0, "left_children": col(0), "loss_changes": [0.0] * n, "parents": col(2),
                "right_children": col(1), "split_conditions": col(4), "split_indices": col(3), "split_type": [0] * n,
                "sum_hessian": [1.0] * n,
                "tree_param": {"num_deleted": "0", "num_feature": str(self.num_feature), "num_nodes": str(n), "size_leaf_vector": "1"}}

    # ---- probes
    def column_specials(self) -> list:
        k = KZERO
        out = [NAN, 0.0, -0.0, 5e-324, -5e-324, 1e-36, -1e-36, k, -k, next_f64(k, True), next_f64(k, False),
               next_f64(-k, True), next_f64(-k, False), self.neutral, self.above]
        if not self.is_xgb:
            out += [INF, -INF, DBL_MAX, -DBL_MAX]
        return out

    def threshold_probes(self, col) -> list:
        """(value, kind, table index) for every entry of the column's table"""
        out = []
        for i, t in enumerate(self.tables[col]):
            t = float(t)
            out += [(t, "t", i), (next_f64(t, False), "prev", i), (next_f64(t, True), "next", i)]
            if self.is_xgb:
                lo, hi = next_f32(t, False), next_f32(t, True)
                mid_lo, mid_hi = (lo + t) / 2, (t + hi) / 2        # exact in f64: the ties of the f64 -> f32 rounding
                out += [(lo, "prev32", i), (hi, "next32", i),
                        (next_f64(mid_lo, True), "narrows-up", i), (next_f64(mid_hi, False), "narrows-down", i),   # both narrow onto t
                        (mid_lo, "tie", i), (mid_hi, "tie", i)]                                                    # ties-to-even
        if self.is_xgb:   # XGBoost rejects a row with a value that narrows to +-inf: the inf case has a test of its own
            out = [p for p in out if np.isfinite(f32(p[0])) or np.isnan(p[0])]
        return out

    def probes(self, n_dense: int = 320):
        """-> (X, meta): X rows x n_cols f64; meta[r] = (column, kind, table index) of a single-column probe (every other column
        holds the neutral value), None for a dense row (every column holds a probe of its own)"""
        rows, meta, pools = [], [], {}
        for c in range(self.n_cols):
            ps = (self.threshold_probes(c) if c in self.tables else []) + [(v, "special", -1) for v in self.column_specials()]
            pools[c] = ps
            for v, kind, i in ps:
                row = np.full(self.n_cols, self.neutral)
                row[c] = v
                rows.append(row)
                meta.append((c, kind, i))
        rng = np.random.Generator(np.random.PCG64([SEED, 7, len(rows)]))
        for _ in range(n_dense):
            rows.append(np.array([pools[c][int(rng.integers(len(pools[c])))][0] for c in range(self.n_cols)]))
            meta.append(None)
        if len(rows) % 128 == 0:   # the whole matrix is the row count "not a multiple of 128, well above 128"
            rows.append(np.full(self.n_cols, self.neutral))
            meta.append((0, "special", -1))
        return np.array(rows, dtype=np.float64), meta

    # ---- references
    def prep(self, x: np.ndarray) -> np.ndarray:
        """what the library does to a dense-row value before any tree sees it"""
        x = np.asarray(x, dtype=np.float64)
        if self.is_xgb:   # ltrlib narrows Double -> Float before the DMatrix
            with np.errstate(over="ignore"):
                return x.astype(np.float32).astype(np.float64)
        return np.where((np.abs(x) > KZERO) | np.isnan(x), x, 0.0)   # RowFunctionFromDenseMatric drops |x| <= kZeroThreshold

    def reference_scores(self, X: np.ndarray) -> np.ndarray:
        """LightGBM Tree::NumericalDecision / XGBoost RegTree::GetNext on the tree descriptions above; sums in tree order, f64
        from 0 for LightGBM, f32 from the base score 0.5 for XGBoost"""
        Xp = self.prep(X)
        acc = np.full(len(X), 0.5, dtype=np.float32) if self.is_xgb else np.zeros(len(X), dtype=np.float64)
        for t in self.trees:
            x = Xp[:, t.col]
            mt, dl = t.rule
            thr = np.array([n[0] for n in t.nodes])
            child = np.array([[n[1], n[2]] for n in t.nodes])
            isn = np.isnan(x)
            if self.is_xgb:
                missing = isn
            else:
                if mt != 2:
                    x = np.where(isn, 0.0, x)     # NaN is compared as 0.0 unless the node's missing type is NaN
                missing = (np.abs(x) <= KZERO) if mt == 1 else np.isnan(x) if mt == 2 else np.zeros(len(x), dtype=bool)
            cur = np.zeros(len(x), dtype=np.int64)
            while (cur >= 0).any():
                at = np.maximum(cur, 0)
                with np.errstate(invalid="ignore"):
                    left = (x < thr[at]) if self.is_xgb else (x <= thr[at])
                left = np.where(missing, dl, left)
                cur = np.where(cur >= 0, child[at, np.where(left, 0, 1)], cur)
            leaf = (~cur).astype(acc.dtype)
            acc = acc + leaf
        return acc.astype(np.float64)

    def expected_bins(self, X: np.ndarray) -> np.ndarray:
        """rows x n_cols: each column's contribution to the score, from the reference evaluator one column at a time"""
        out = np.zeros(X.shape)
        base = self.reference_scores(np.full((1, self.n_cols), self.neutral))[0]
        for c in self.split_cols:
            Y = np.full(X.shape, self.neutral)
            Y[:, c] = X[:, c]
            out[:, c] = self.reference_scores(Y) - base
        return out

    def column_has_zero_rule(self, col) -> bool:
        return any(t.col == col and t.rule[0] == 1 for t in self.trees)

    def searchsorted_bins(self, X: np.ndarray, meta: list):
        """(row indices, bins): np.searchsorted on the single-column probes whose value is not missing in its column"""
        idx, out = [], []
        for r, m in enumerate(meta):
            if m is None or m[0] not in self.tables:
                continue
            c = m[0]
            x = float(self.prep(X[r, c:c + 1])[0])
            if np.isnan(x) or (x == 0.0 and self.column_has_zero_rule(c)):
                continue
            idx.append(r)
            out.append(int(np.searchsorted(self.tables[c], x, side="right" if self.is_xgb else "left")))
        return np.array(idx), np.array(out, dtype=np.float64)

    # ---- failures
    def explain(self, X, meta, got, exp, limit=8) -> str:
        """the rows whose score differs: column, probe value as hex, expected bin, bin decoded from the score"""
        bad = np.flatnonzero(~((got == exp) | (np.isnan(got) & np.isnan(exp))))
        base = 0.5 if self.is_xgb else 0.0
        lines = [f"{len(bad)} of {len(exp)} rows differ ({self.backend} layout {self.layout})"]
        for r in bad[:limit]:
            m = meta[r]
            if m is not None:
                c, kind, i = m
                lines.append(f"  row {r}: column {c} (table of {self.lengths.get(c, 0)}), probe {kind}[{i}] = {float(X[r, c]).hex()}: "
                             f"expected bin {exp[r] - base:g}, bin decoded from the score {got[r] - base:g}")
            else:
                eb = self.expected_bins(X[r:r + 1])[0]
                cells = ", ".join(f"c{c}={float(X[r, c]).hex()}->bin {eb[c]:g}" for c in self.split_cols)
                lines.append(f"  dense row {r}: expected sum of bins {exp[r] - base:g}, got {got[r] - base:g}; per column: {cells}")
        return "\n".join(lines)


# the (layout, backend, rules) cases of both test files
CASES = [(lay, be, "per_feature") for lay in ("S", "M", "L") for be in ("lgbm", "xgb")] + [("M", "lgbm", "per_tree")]
_cache: dict = {}


def case(layout, backend, rules="per_feature"):
    """-> (forest, X, meta, reference scores): built once per process"""
    key = (layout, backend, rules)
    if key not in _cache:
        f = BoundaryForest(layout, backend, rules)
        X, meta = f.probes()
        _cache[key] = (f, X, meta, f.reference_scores(X))
    return _cache[key]
