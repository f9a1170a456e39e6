"""GPU: the similar-items fit on the device (csrc/als.hip through mrk_als_*) against the loop form of the Python restatement
(tests/als_reference.py): item factors - and user factors where asked for - must have its BIT PATTERNS.  Shapes are the smallest
at which each piece can go wrong: the edges of the 64-lane grouping of the factor loop and of a row's entries, rows on both sides of
the LDS staging threshold (lowered by MRK_ALS_STAGE_MAX), more than one chunk of the K x K products."""
import ctypes as C
import os

import numpy as np
import pytest

import als_reference as A
import metarank_amd as M
from metarank_amd import _native as N
from metarank_amd.als import AlsBuilder, init_matrix
from metarank_amd.index import HipIndex

pytestmark = pytest.mark.gpu


@pytest.fixture
def stage_env():
    saved = os.environ.get("MRK_ALS_STAGE_MAX")
    yield
    if saved is None:
        os.environ.pop("MRK_ALS_STAGE_MAX", None)
    else:
        os.environ["MRK_ALS_STAGE_MAX"] = saved
    M.reload_switches()


def stream(seed, n, users, items):
    """n random pairs in which every user and every item appears"""
    rng = np.random.default_rng(seed)
    m = max(users, items)
    u = np.concatenate([np.arange(m) % users, rng.integers(0, users, n - m)])
    i = np.concatenate([np.arange(m) % items, rng.integers(0, items, n - m)])
    order = rng.permutation(n)
    return [f"user-{v}" for v in u[order]], [f"item-{v}" for v in i[order]]


def device_fit(ctx, config, us, its, seed=0, init=None, batches=1):
    """(item ids, item factors, user factors, index info) of a fit on the device"""
    b = AlsBuilder(config, ctx)
    try:
        cuts = [len(us) * k // batches for k in range(batches + 1)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            b.add(us[lo:hi], its[lo:hi])
        ix, P = b.fit(seed=seed, init=init, user_factors=True)
        try:
            return ix.ids(), ix.vectors(), P, ix.info()
        finally:
            ix.close()
    finally:
        b.close()


def check(ctx, config, us, its, init_seed=1, batches=1):
    """fits on the device and by the loop form from the same initial matrices; returns the device's (P, Q)"""
    pr = A.Problem(us, its)
    cfg = A.parse_config(config)
    K = cfg["factors"]
    P0, Q0 = init_matrix(init_seed, 0, len(pr.users), K), init_matrix(init_seed, 1, len(pr.items), K)
    want_P, want_Q = A.fit_loop(cfg, pr, P0, Q0)
    ids, Q, P, info = device_fit(ctx, config, us, its, init=(P0, Q0), batches=batches)
    assert ids == pr.items
    assert info["rows"] == len(pr.items) and info["cols"] == K and info["stored_elem_bytes"] == 8
    assert np.array_equal(A.bits(Q), A.bits(want_Q)), float(np.abs(Q - want_Q).max())
    assert np.array_equal(A.bits(P), A.bits(want_P)), float(np.abs(P - want_P).max())
    assert np.isfinite(Q).all()
    return P, Q


def status_of(fn):
    with pytest.raises(N.MrkError) as e:
        fn()
    return e.value.status


def test_hand_written_case(ctx):
    """3 users x 4 items, K = 2, one iteration from hand-written factors"""
    us = ["a", "a", "b", "b", "b", "c"]
    its = ["w", "x", "x", "y", "z", "w"]
    P0 = np.array([[0.1, -0.2], [0.3, 0.05], [-0.15, 0.25]])
    Q0 = np.array([[0.2, 0.1], [-0.1, 0.3], [0.05, -0.25], [0.4, 0.0]])
    cfg = {"factors": 2, "iterations": 1}
    want_P, want_Q = A.fit_loop(A.parse_config(cfg), A.Problem(us, its), P0, Q0)
    ids, Q, P, info = device_fit(ctx, cfg, us, its, init=(P0, Q0))
    assert ids == ["w", "x", "y", "z"] and info["stored_elem_bytes"] == 8
    assert np.array_equal(A.bits(Q), A.bits(want_Q)) and np.array_equal(A.bits(P), A.bits(want_P))
    assert not np.array_equal(Q, Q0)


@pytest.mark.parametrize("K", [1, 3, 64, 65, 100])
def test_factor_counts(ctx, K):
    """the edges of the 64-lane grouping of the k-sum and of the lanes that own a factor"""
    us, its = stream(K, 260, 40, 25)
    check(ctx, {"factors": K, "iterations": 2, "userReg": 0.05, "itemRef": 0.02}, us, its)


def long_rows():
    """users with 1, 63, 64, 65 and 130 items, items with 1, 63, 64, 65 and 130 users"""
    us, its = [], []
    for n in (1, 63, 64, 65, 130):
        us += [f"U{n}"] * n
        its += [f"i{k}" for k in range(n)]
        us += [f"u{k}" for k in range(n)]
        its += [f"I{n}"] * n
    return us, its


def test_row_lengths_on_both_sides_of_the_staging_threshold(ctx, stage_env):
    """With 8 staged entries at the most, the rows of 63 ... 130 entries gather their factor rows from memory at every step; with the
    default (every row of this input staged) the bytes must be the same: the order of a sum does not depend on the path its row took"""
    us, its = long_rows()
    cfg = {"factors": 5, "iterations": 2}
    os.environ["MRK_ALS_STAGE_MAX"] = "8"
    M.reload_switches()
    P_low, Q_low = check(ctx, cfg, us, its)
    os.environ.pop("MRK_ALS_STAGE_MAX")
    M.reload_switches()
    P_dflt, Q_dflt = check(ctx, cfg, us, its)
    assert P_low.tobytes() == P_dflt.tobytes() and Q_low.tobytes() == Q_dflt.tobytes()


def test_a_user_with_every_item_and_many_users_with_one_entry(ctx):
    """1 100 users with a single entry (three chunks of the product over the users), one user who has all 7 items, one item with one user"""
    rng = np.random.default_rng(5)
    us = [f"single-{k}" for k in range(1100)] + ["everything"] * 7
    its = [f"i{v}" for v in rng.integers(0, 6, 1100)] + [f"i{k}" for k in range(7)]
    pr = A.Problem(us, its)
    assert len(pr.item_rows[pr.items.index("i6")]) == 1 and len(pr.user_rows[pr.users.index("everything")]) == len(pr.items) == 7
    check(ctx, {"factors": 3, "iterations": 1}, us, its)


def test_duplicates_cuts_and_repeated_fits_leave_the_bytes_unchanged(ctx):
    us, its = stream(21, 300, 30, 20)
    cfg = {"factors": 4, "iterations": 2}
    _, Q = check(ctx, cfg, us, its)
    _, Q_cut = check(ctx, cfg, us, its, batches=7)
    assert Q.tobytes() == Q_cut.tobytes()
    pr = A.Problem(us, its)
    P0, Q0 = init_matrix(1, 0, len(pr.users), 4), init_matrix(1, 1, len(pr.items), 4)
    b = AlsBuilder(cfg, ctx)
    b.add(us, its)
    first = b.fit(init=(P0, Q0))
    second = b.fit(init=(P0, Q0))
    b.add(us[::-1][:100], its[::-1][:100])           # pairs that are all there already
    assert b.info()["pairs"] == 400 and b.info()["distinct_pairs"] == pr.nnz
    third = b.fit(init=(P0, Q0))
    for ix in (first, second, third):
        assert ix.vectors().tobytes() == Q.tobytes()
        ix.close()
    b.close()


def test_a_seeded_fit_equals_a_fit_from_the_generators_matrices(ctx):
    us, its = stream(22, 200, 25, 15)
    cfg = {"factors": 6, "iterations": 2}
    pr = A.Problem(us, its)
    _, Q_seed, P_seed, _ = device_fit(ctx, cfg, us, its, seed=77)
    init = (init_matrix(77, 0, len(pr.users), 6), init_matrix(77, 1, len(pr.items), 6))
    _, Q_init, P_init, _ = device_fit(ctx, cfg, us, its, seed=5, init=init)
    assert Q_seed.tobytes() == Q_init.tobytes() and P_seed.tobytes() == P_init.tobytes()
    _, Q_other, _, _ = device_fit(ctx, cfg, us, its, seed=78)
    assert Q_other.tobytes() != Q_seed.tobytes()
    ix = HipIndex.fit_similar(cfg, us, its, ctx=ctx, seed=77, batches=3)
    assert ix.vectors().tobytes() == Q_seed.tobytes()
    ix.close()


def test_planted_structure(ctx):
    """two disjoint groups of 20 users x 15 items (als_reference.PLANTED, which the restatement alone passes on the CPU): every item's 5
    nearest neighbours by mrk_index_lookup lie in its own group"""
    us, its = A.planted(A.PLANTED["seed"], density=A.PLANTED["density"])
    cfg = {"factors": A.PLANTED["K"], "iterations": A.PLANTED["iterations"]}
    ix = HipIndex.fit_similar(cfg, us, its, ctx=ctx, seed=A.PLANTED["init_seed"])
    try:
        ids = ix.ids()
        assert len(ids) == 30
        for row, item in enumerate(ids):
            rows, _ = ix.lookup([item], 6)
            near = [r for r in rows.tolist() if r != row][:5]
            assert len(near) == 5 and all(ids[r].split("-")[0] == item.split("-")[0] for r in near), (item, [ids[r] for r in near])
        assert A.planted_neighbours_hold(ids, ix.vectors())
    finally:
        ix.close()


def test_recommend_end_to_end(ctx):
    """mrk_index_recommend on the fitted index = mrk_index_recommend on an index that mrk_index_build makes of the restatement's factors"""
    us, its = stream(23, 400, 40, 30)
    cfg = {"factors": 7, "iterations": 3}
    pr = A.Problem(us, its)
    K = 7
    _, want_Q = A.fit_loop(A.parse_config(cfg), pr, A.init_matrix(3, 0, len(pr.users), K), A.init_matrix(3, 1, len(pr.items), K))
    fitted = HipIndex.fit_similar(cfg, us, its, ctx=ctx, seed=3)
    built = HipIndex.build(pr.items, want_Q, ctx)
    try:
        assert fitted.info()["stored_elem_bytes"] == 8 and fitted.info()["rows"] == len(pr.items) and fitted.ids() == pr.items
        for request in ([pr.items[0]], [pr.items[3], pr.items[11]], [pr.items[-1], "unknown", pr.items[5]]):
            got_rows, got_score = fitted.recommend(request, 10)
            want_rows, want_score = built.recommend(request, 10)
            assert got_rows.tolist() == want_rows.tolist() and len(got_rows) == 10
            assert np.array_equal(A.bits(got_score), A.bits(want_score))
        assert status_of(lambda: fitted.recommend([], 5)) == N.ERR_INVALID_ARG      # MFRecommenderTest: a request without items fails
    finally:
        fitted.close()
        built.close()


def test_errors_leave_the_builder_usable(ctx):
    b = AlsBuilder({"factors": 3, "iterations": 1}, ctx)
    assert status_of(b.fit) == N.ERR_NOT_FOUND
    us, its = stream(24, 60, 10, 8)
    b.add(us, its)
    pr = A.Problem(us, its)
    P0, Q0 = init_matrix(1, 0, len(pr.users), 3), init_matrix(1, 1, len(pr.items), 3)
    assert status_of(lambda: b.fit(init=(P0, None))) == N.ERR_INVALID_ARG
    assert status_of(lambda: b.fit(init=(None, Q0))) == N.ERR_INVALID_ARG
    ix = b.fit(init=(P0, Q0))
    _, want_Q = A.fit_loop(A.parse_config({"factors": 3, "iterations": 1}), pr, P0, Q0)
    assert np.array_equal(A.bits(ix.vectors()), A.bits(want_Q))
    ix.close()
    b.close()
    big = AlsBuilder({"factors": A.MAX_FACTORS + 1, "iterations": 1}, ctx)
    big.add(us, its)
    with pytest.raises(N.MrkError) as e:
        big.fit()
    assert e.value.status == N.ERR_UNSUPPORTED and str(A.MAX_FACTORS + 1) in e.value.message and str(A.MAX_FACTORS) in e.value.message
    assert big.info()["pairs"] == 60
    h = C.c_void_p()
    assert N.lib().mrk_als_fit(big._h, 0, None, None, None, C.byref(h)) == N.ERR_UNSUPPORTED and not h.value
    big.close()
