"""GPU: the trending recommender's fit on the device (csrc/trending.hip through mrk_trending_*) against the scalar Python
restatement of TrendingPredictor.fit (tests/trending_reference.py): ids, order and score BIT PATTERNS must be equal.  Decays
come from {1.0, 0.5, 2.0, 0.25, 0.0, 1e200} - their powers are exact, or overflow to Infinity, in any correctly rounded pow -
except in the one test that says otherwise.  Shapes are the smallest at which each piece can go wrong."""
import numpy as np
import pytest

import trending_reference as T
from metarank_amd import _native as N
from metarank_amd.trending import HipTrending, TrendingBuilder

pytestmark = pytest.mark.gpu

DAY = T.DAY_MS
NOW = 1_700_000_000_000


def check(ctx, config, ids, types, ts, batches=1):
    """fits on the device and by the restatement; returns the model's (ids, scores)"""
    want_ids, want_scores = T.fit(config, ids, types, ts)
    m = HipTrending.fit(config, ids, types, ts, ctx=ctx, batches=batches)
    try:
        assert m.info() == {"items": len(want_ids), "interactions": len(ids), "now_ms": max(ts)}
        got_ids, got_scores = m.predict(len(want_ids) + 5)
        assert got_ids == want_ids
        assert T.bits(got_scores).tolist() == T.bits(want_scores).tolist()
        assert m.save() == T.save(want_ids, want_scores) or np.isnan(want_scores).any()   # (a NaN's payload is the device's own)
    finally:
        m.close()
    return got_ids, got_scores


def status_of(fn):
    with pytest.raises(N.MrkError) as e:
        fn()
    return e.value.status


@pytest.mark.parametrize("name", sorted(T.KNOWN_ANSWERS))
def test_known_answers(ctx, name):
    """TrendingRecommenderTest.scala:28-72 on the device"""
    ids, types, ts, want = T.KNOWN_ANSWERS[name]
    got_ids, got_scores = check(ctx, T.TEST_CONFIG, ids, types, ts)
    assert list(zip(got_ids, got_scores.tolist())) == want


def history(n_items, n_interactions, seed, span_days=30):
    """every item at least once, in a shuffled order of first appearance; types click / buy / other; ts in (NOW - span, NOW]"""
    rng = np.random.default_rng(seed)
    item = np.concatenate([rng.permutation(n_items), rng.integers(0, n_items, max(n_interactions - n_items, 0))])[:max(n_interactions, 1)]
    if n_interactions >= n_items:
        rng.shuffle(item)
    types = rng.choice(["click", "click", "buy", "other"], len(item)).tolist()
    ts = (NOW - rng.integers(0, span_days * DAY, len(item))).tolist()
    ts[int(rng.integers(0, len(item)))] = NOW
    return [f"i{v}" for v in item], types, ts


@pytest.mark.parametrize("n_items", [1, 63, 64, 65, 255, 256, 257, 4096, 4097, 8200])
def test_item_counts(ctx, n_items):
    """wavefront / workgroup edges of the score kernel, the switch from the one-workgroup order to the big sort"""
    decays = [1.0, 0.5, 2.0, 0.25]
    cfg = {"weights": [{"interaction": "buy", "weight": 5.0, "decay": decays[n_items % 4], "window": "1d"},
                       {"interaction": "click", "weight": 0.5, "decay": decays[(n_items // 4 + 1) % 4], "window": "30d"}]}
    ids, types, ts = history(n_items, 4 * n_items, seed=n_items)
    got_ids, _ = check(ctx, cfg, ids, types, ts)
    assert len(got_ids) == n_items


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_interaction_counts(ctx, n):
    """grid-stride edges of the count kernel: 10 items (fewer interactions than items: the items seen)"""
    cfg = {"weights": [{"interaction": "click", "decay": 0.5}, {"interaction": "buy", "weight": 3.0, "decay": 2.0, "window": "7d"}]}
    ids, types, ts = history(10, n, seed=100 + n)
    check(ctx, cfg, ids, types, ts)


def test_contention(ctx):
    """20 000 interactions on ONE bin (the wavefront-combined atomic), 3 cold items; the same volume over 2 items x 2 days"""
    cfg = {"weights": [{"interaction": "click", "weight": 3.0, "decay": 0.5}]}
    ids = ["cold1", "hot"] + ["hot"] * 19_999 + ["cold2", "cold3"]
    types = ["click"] * len(ids)
    ts = [NOW - 5 * DAY] + [NOW - k % 1000 for k in range(20_000)] + [NOW - DAY, NOW - 29 * DAY]
    got_ids, got_scores = check(ctx, cfg, ids, types, ts)
    assert got_ids[0] == "hot" and got_scores[0] == 20_000.0 * 3.0
    ids = [("a", "b")[k % 2] for k in range(20_000)]
    ts = [NOW - (k // 2 % 2) * DAY - k % 777 for k in range(20_000)]
    got_ids, got_scores = check(ctx, cfg, ids, ["click"] * 20_000, ts)
    assert got_ids == ["a", "b"] and got_scores.tolist() == [(5000.0 + 5000.0 * 0.5) * 3.0] * 2


def test_window_edges(ctx):
    cfg = {"weights": [{"interaction": "click", "decay": 2.0, "window": "4d"}]}
    ids = ["at_window", "just_inside", "k2", "k2_minus_1ms", "k1", "today", "mover"]
    ts = [NOW - 4 * DAY, NOW - 4 * DAY + 1, NOW - 2 * DAY, NOW - 2 * DAY + 1, NOW - DAY, NOW - 1, NOW]
    types = ["click"] * 6 + ["view"]     # `view` is named by no weight: it carries the maximal ts, so it moves `now`, and its item scores 0.0
    got_ids, got_scores = check(ctx, cfg, ids, types, ts)
    score = dict(zip(got_ids, got_scores.tolist()))
    assert score == {"at_window": 0.0, "just_inside": 8.0, "k2": 4.0, "k2_minus_1ms": 2.0, "k1": 2.0, "today": 1.0, "mover": 0.0}
    assert got_ids == ["just_inside", "k2", "k2_minus_1ms", "k1", "today", "at_window", "mover"]
    # without the mover `now` is one ms earlier: every bucket edge moves with it
    got_ids, got_scores = check(ctx, cfg, ids[:6], types[:6], ts[:6])
    assert dict(zip(got_ids, got_scores.tolist())) == {"at_window": 8.0, "just_inside": 8.0, "k2": 2.0, "k2_minus_1ms": 2.0, "k1": 1.0, "today": 1.0}


def test_ties_keep_first_appearance_across_the_sort_boundary(ctx):
    cfg = {"weights": [{"interaction": "click"}]}
    for n in (4096, 4097, 5000):
        ids = [f"t{(k * 7919) % n}" for k in range(n)]          # 7919 is prime to each n: a permutation
        assert len(set(ids)) == n
        ids2 = ids + ids[100:200]                               # 100 items score 2.0, in their order of first appearance, before the rest
        got_ids, got_scores = check(ctx, cfg, ids2, ["click"] * len(ids2), [NOW - k % 5 for k in range(len(ids2))])
        assert got_ids == ids[100:200] + ids[:100] + ids[200:]


def test_negative_weight_and_signed_zeros(ctx):
    cfg = {"weights": [{"interaction": "click", "weight": -1.0, "decay": 0.0, "window": "2d"}]}
    ids = ["minus_zero", "minus_one", "plus_zero", "minus_two", "minus_two", "minus_zero2"]
    types = ["click", "click", "view", "click", "click", "click"]
    ts = [NOW - DAY, NOW, NOW, NOW, NOW - 5, NOW - DAY - 1]
    got_ids, got_scores = check(ctx, cfg, ids, types, ts)         # decay 0.0: pow(0, 0) = 1, pow(0, 1) = 0 -> yesterday counts 1 * 0.0, times -1 = -0.0
    assert got_ids == ["plus_zero", "minus_zero", "minus_zero2", "minus_one", "minus_two"]
    assert T.bits(got_scores).tolist() == T.bits(np.array([0.0, -0.0, -0.0, -1.0, -2.0])).tolist()
    # a LEADING part of -0.0 stays -0.0 when +0.0 parts follow only if the sum starts from it ... and -0.0 + 0.0 is +0.0 anyway
    cfg2 = {"weights": [cfg["weights"][0], {"interaction": "buy"}]}
    got_ids, got_scores = check(ctx, cfg2, ids, types, ts)
    assert T.bits(got_scores[:3]).tolist() == [0, 0, 0] and got_ids[:3] == ["minus_zero", "plus_zero", "minus_zero2"]


def test_infinite_powers_give_nan_and_nan_sorts_last(ctx):
    cfg = {"weights": [{"interaction": "click", "decay": 1e200, "window": "3d"}]}
    ids = ["nan1", "inf", "inf", "finite_none", "nan2", "big", "big"]
    types = ["click", "click", "click", "view", "click", "click", "click"]
    ts = [NOW, NOW, NOW - 2 * DAY, NOW, NOW - DAY, NOW - 2 * DAY, NOW - 2 * DAY - 5]
    got_ids, got_scores = check(ctx, cfg, ids, types, ts)
    # nan1 / nan2: a count of 0 in bucket 2 times Infinity; inf / big: a count there; finite_none: no counted interaction, +0.0
    assert got_ids == ["inf", "big", "finite_none", "nan1", "nan2"]
    assert got_scores[0] == np.inf and got_scores[1] == np.inf and got_scores[2] == 0.0 and np.isnan(got_scores[3:]).all()


def test_refusals(ctx):
    cfg = {"weights": [{"interaction": "click", "window": "36h"}]}
    fit = lambda ids, ts: HipTrending.fit(cfg, ids, ["click"] * len(ids), ts, ctx=ctx)
    assert status_of(lambda: fit(["a", "b"], [NOW, NOW - 30 * 3_600_000])) == N.ERR_DIM_MISMATCH      # bucket 1 of a one-day array
    check(ctx, cfg, ["a", "b", "c"], ["click"] * 3, [NOW, NOW - 23 * 3_600_000, NOW - 40 * 3_600_000])  # nothing inside the window is older than a day
    assert status_of(lambda: fit([], [])) == N.ERR_NOT_FOUND
    sub_day = {"weights": [{"interaction": "click", "window": "12h"}]}                                # days = 0: any counted interaction is outside
    assert status_of(lambda: HipTrending.fit(sub_day, ["a"], ["click"], [NOW], ctx=ctx)) == N.ERR_DIM_MISMATCH
    check(ctx, sub_day, ["a"], ["view"], [NOW])
    m = fit(["a"], [NOW])
    assert status_of(lambda: m.predict(0)) == N.ERR_INVALID_ARG and status_of(lambda: m.predict(-1)) == N.ERR_INVALID_ARG
    m.close()
    # an index outside the call's type table: the call fails and nothing of it is appended
    import ctypes as C
    b = TrendingBuilder(cfg, ctx)
    b.add(["a", "b"], ["click", "click"], [NOW, NOW - 5])
    ids = (C.c_char_p * 2)(b"zz", b"yy")
    names = (C.c_char_p * 1)(b"click")
    idx = np.array([0, 1], dtype=np.int32)
    ts = np.array([NOW + 99, NOW + 99], dtype=np.int64)
    assert N.lib().mrk_trending_add(b._h, ids, names, 1, idx.ctypes.data, ts.ctypes.data, 2) == N.ERR_INVALID_ARG
    m = b.fit()
    assert m.items() == ["a", "b"] and m.info()["now_ms"] == NOW and m.info()["interactions"] == 2
    m.close()
    b.close()


def test_batching_does_not_change_the_bytes(ctx):
    cfg = {"weights": [{"interaction": "buy", "weight": 5.0, "decay": 0.5, "window": "7d"}, {"interaction": "click", "decay": 0.25}]}
    ids, types, ts = history(300, 2000, seed=9)
    want = T.save(*T.fit(cfg, ids, types, ts))
    for batches in (1, 2, 7):
        m = HipTrending.fit(cfg, ids, types, ts, ctx=ctx, batches=batches)
        assert m.save() == want, batches
        m.close()
    # a second fit after more adds equals a fresh fit of the whole stream; calls may carry different type tables
    b = TrendingBuilder(cfg, ctx)
    b.add(ids[:900], types[:900], ts[:900])
    first = b.fit()
    assert first.save() == T.save(*T.fit(cfg, ids[:900], types[:900], ts[:900]))
    b.add(ids[900:], types[900:], ts[900:])
    second = b.fit()
    assert second.save() == want and first.info()["interactions"] == 900
    for m in (first, second):
        m.close()
    b.close()


def test_inexact_powers_follow_the_host_libm(ctx):
    """decay 0.9: its powers are not exactly representable, so this pins library == host libm (the pow the restatement's
    math.pow calls too) - NOT the JVM's Math.pow, which cannot be run here (unpinned)"""
    cfg = {"weights": [{"interaction": "click", "weight": 1.5, "decay": 0.9}]}
    ids, types, ts = history(100, 1000, seed=4)
    check(ctx, cfg, ids, types, ts)


def test_plain_count_form_gives_the_same_bytes(ctx, monkeypatch):
    """MRK_TRENDING_COUNT=plain (one atomic per interaction, the other arm of the count kernel's A/B; read at each fit)
    counts the same table: hot bins, cold bins, several wavefronts and workgroups"""
    cfg = {"weights": [{"interaction": "buy", "weight": 5.0, "decay": 0.5, "window": "7d"}, {"interaction": "click", "decay": 0.25}]}
    ids, types, ts = history(300, 3000, seed=21)
    ids, types, ts = ids + ["hot"] * 2000, types + ["click"] * 2000, ts + [NOW - k % 50 for k in range(2000)]
    want = T.save(*T.fit(cfg, ids, types, ts))
    for mode in ("plain", "combine"):
        monkeypatch.setenv("MRK_TRENDING_COUNT", mode)
        m = HipTrending.fit(cfg, ids, types, ts, ctx=ctx)
        assert m.save() == want, mode
        m.close()


def test_an_id_too_long_for_writeutf_fits_but_does_not_save(ctx):
    """rule 9 through the C ABI: 65 535 bytes save, 65 536 are what writeUTF throws on - MRK_ERR_UNSUPPORTED; predict and id still serve it"""
    cfg = {"weights": [{"interaction": "click"}]}
    ok, long_id = "y" * 65535, "x" * 65536
    m = HipTrending.fit(cfg, ["a", ok, ok], ["click"] * 3, [NOW] * 3, ctx=ctx)
    assert m.save() == T.save([ok, "a"], [2.0, 1.0])
    m.close()
    m = HipTrending.fit(cfg, ["a", long_id, long_id], ["click"] * 3, [NOW] * 3, ctx=ctx)
    assert status_of(m.save) == N.ERR_UNSUPPORTED
    got_ids, got_scores = m.predict(2)
    assert got_ids == [long_id, "a"] and got_scores.tolist() == [2.0, 1.0]
    m.close()


def test_no_weights_at_all(ctx):
    """rule 6: an empty weights list - no count table, no pow table - scores every item +0.0 in order of first appearance"""
    got_ids, got_scores = check(ctx, {"weights": []}, ["b", "a", "b", "c"], ["click", "buy", "click", "view"], [NOW - 5, NOW, NOW - DAY, NOW - 40 * DAY])
    assert got_ids == ["b", "a", "c"] and T.bits(got_scores).tolist() == [0, 0, 0]
