"""The boundary grid of tests/boundary_forests.py on the CPU: the numpy reference evaluator, np.searchsorted and the oracle
(oracle/forest_oracle.cpp) agree exactly on every probe - the oracle pinned, on threshold-adjacent values, against something
that is not our own C++ - and the grid covers what it claims to cover (conditions, not measurements)."""
import numpy as np
import pytest

import boundary_forests as bf
from oracle.forest import OracleForest


def oracle_of(f):
    blob = f.model_bytes()
    return OracleForest.from_xgboost(blob) if f.is_xgb else OracleForest.from_lightgbm_text(blob)


@pytest.mark.parametrize("layout,backend,rules", bf.CASES)
def test_reference_searchsorted_and_oracle_agree(layout, backend, rules):
    f, X, meta, ref = bf.case(layout, backend, rules)
    base = 0.5 if f.is_xgb else 0.0
    # the neutral value is below every table and not missing: a single-column probe's score is its column's bin
    assert f.reference_scores(np.full((1, f.n_cols), f.neutral))[0] == base
    idx, bins = f.searchsorted_bins(X, meta)
    assert len(idx) > 3 * sum(f.lengths.values())
    assert np.array_equal(ref[idx], bins + base), f.explain(X[idx], [meta[i] for i in idx], bins + base, ref[idx])
    got = oracle_of(f).predict(X)
    assert np.array_equal(got, ref), f.explain(X, meta, got, ref)
    # columns the forest never splits on, and the one beyond num_feature, contribute nothing whatever they hold
    for r, m in enumerate(meta):
        if m is not None and m[0] in f.unsplit_cols:
            assert ref[r] == base, (r, m)


@pytest.mark.parametrize("layout,backend,rules", bf.CASES)
def test_grid_coverage(layout, backend, rules):
    f, X, meta, ref = bf.case(layout, backend, rules)
    base = 0.5 if f.is_xgb else 0.0
    assert X.shape[1] == f.n_cols == f.num_feature + 1 and len(X) % 128 != 0 and len(X) > 1000
    assert sorted(f.lengths.values()) == sorted([n for n in bf.LAYOUTS[layout] if n != "U"] + ([bf.XGB_EXTRA] if f.is_xgb else []))
    assert 24 <= f.n_cols <= 30
    # a never-split column lies between split-on columns
    assert any(f.split_cols[0] < c < f.split_cols[-1] for c in f.unsplit_cols)
    hit = {}
    bins_seen = {c: set() for c in f.split_cols}
    idx, bins = f.searchsorted_bins(X, meta)
    for r, b in zip(idx, bins):
        bins_seen[meta[r][0]].add(int(b))
    for r, m in enumerate(meta):
        if m is not None and m[2] >= 0:
            hit.setdefault((m[0], m[2]), set()).add(m[1])
            # the probe's bit pattern is what the table entry says it is
            t = float(f.tables[m[0]][m[2]])
            want = {"t": t, "prev": bf.next_f64(t, False), "next": bf.next_f64(t, True)}.get(m[1])
            if want is not None:
                assert bf.bits([X[r, m[0]]])[0] == bf.bits([want])[0]
    for c in f.split_cols:
        T = f.tables[c]
        assert len(np.unique(T)) == f.lengths[c]
        for i in range(len(T)):
            assert {"t", "prev", "next"} <= hit[(c, i)], (c, i)     # every (column, table index): t, prev and next
        # every bin 0..len that any value can reach: none lies between -0.0 and 0.0, and LightGBM flushes |x| <= 1e-35f to 0.0
        # before any tree sees it, so thresholds inside the flush are only ever separated by 0.0 itself - which is "missing", not a
        # bin, in a column with a Zero-type rule
        lo = np.concatenate([[-bf.INF], T])
        hi = np.concatenate([T, [bf.INF]])
        empty = {k for k in range(len(T) + 1) if lo[k] == hi[k]}
        if not f.is_xgb:
            empty |= {k for k in range(len(T) + 1) if lo[k] >= -bf.KZERO and hi[k] <= bf.KZERO and (f.column_has_zero_rule(c) or not lo[k] < 0.0 <= hi[k])}
        assert bins_seen[c] == set(range(len(T) + 1)) - empty, c
        assert len(empty) <= 7
    # -0.0 and the denormals survive into the matrix
    ub = set(bf.bits(X).ravel().tolist())
    for v in (-0.0, 0.0, 5e-324, -5e-324, 1e-36, -1e-36, bf.KZERO, -bf.KZERO):
        assert int(bf.bits([v])[0]) in ub, v
    assert np.isnan(X).any()
    # every tree is within the bit-vector scorer's limits, and full 16-leaf trees exist where a table has 15 entries
    assert max(t.n_leaves for t in f.trees) == (16 if max(f.lengths.values()) >= 15 else max(f.lengths.values()) + 1)
    rules_used = {t.rule for t in f.trees}
    assert rules_used == set(bf.XGB_RULES if f.is_xgb else bf.LGBM_RULES)
    if rules == "per_tree":   # a column carries several views
        assert max(len({t.rule for t in f.trees if t.col == c}) for c in f.split_cols) >= 4
    assert ref.min() >= base and ref.max() > 255


def test_layouts_cover_the_structural_edges():
    lengths, mods, specials = set(), set(), set()
    for layout, backend, rules in bf.CASES:
        f = bf.case(layout, backend, rules)[0]
        lengths |= set(f.lengths.values())
        mods.add(len(f.split_cols) % 4)
        for T in f.tables.values():
            specials |= set(bf.bits(T).tolist())
        for T in f.tables.values():   # two thresholds that are adjacent doubles / floats
            if f.is_xgb and any(bf.next_f32(a, True) == b for a, b in zip(T[:-1], T[1:]) if a != 0 and abs(a) > 1e-30):
                specials.add("adjacent32")
            if not f.is_xgb and any(bf.next_f64(a, True) == b for a, b in zip(T[:-1], T[1:]) if abs(a) > 1e-30):
                specials.add("adjacent64")
    assert set(bf.ALL_LENGTHS) <= lengths and max(lengths) >= 513
    assert mods == {0, 1, 2, 3}                    # CellSinkRT::finish()'s group shapes
    want = [0.0, -0.0, 1e-36, -1e-36, 1e-37, -1e-37, bf.KZERO, -bf.KZERO, bf.DBL_MAX, -bf.DBL_MAX, bf.FLT_MAX, bf.FLT_DENORM]
    for v in want:
        assert int(bf.bits([v])[0]) in specials, v
    assert {"adjacent32", "adjacent64"} <= specials
    # residency classes (doubles of the distinct tables of at most 256 entries): S resident everywhere (<= 8 KB), M staged by the
    # fused kernel and resident in the split kernel (8 KB .. 20 KB), S and M byte-eligible (k <= 254), L not
    for backend in ("lgbm", "xgb"):
        tot = {lay: sum(n for n in bf.case(lay, backend)[0].lengths.values() if n <= 256) for lay in "SML"}
        assert tot["S"] * 8 <= 8192 < tot["M"] * 8 <= 20480 and tot["L"] * 8 > 8192
        assert max(bf.case("S", backend)[0].lengths.values()) <= 255 == max(bf.case("M", backend)[0].lengths.values())
        assert max(bf.case("L", backend)[0].lengths.values()) >= 513
