"""The device median of a numeric `diversity` over more values than the pre-pass sorts in LDS (csrc/select.hip: gather + radix
select, taken whenever min(top, n_items) > 4 096) against the oracle's sorted-array restatement of commons-math's LEGACY
percentile (DiversityFeature.scala:113-126), bit for bit, through mrk_batch_* with host-resolved and with flat (device-resolved)
ids; the "median" timer; and MRK_DIVERSITY_SELECT=0, the host's walk + sort, giving the same bits."""
import os

import numpy as np
import pytest

import metarank_amd as M
from backends import HipBackend, OracleBackend, single_feature_config
from workloads import ranklens

INF, NAN = float("inf"), float("nan")


def shuffled(vals, seed):
    return list(np.random.default_rng(seed).permutation(np.array(vals, dtype=np.float64)))


def normal(n, seed):
    return list(np.random.default_rng(seed).normal(size=n).round(3))


# name -> (state of candidate i: a float, a str or None = no state; top; sizes of the requests, each the first n candidates)
CASES = {
    "4097 values, m odd": (normal(4097, 1), 100000, [4097]),
    "4098 values, m even": (normal(4098, 2), 100000, [4098]),
    "holes, top cuts inside the request": ([None if i % 17 == 5 else v for i, v in enumerate(normal(6000, 3))], 5000, [6000]),
    "-0.0 and +0.0 in the middle": (shuffled(list(-1.0 - np.arange(2048)) + [-0.0, 0.0] + list(1.0 + np.arange(2048)), 4), 100000, [4098]),
    "3000 copies of the median": (shuffled([1.5] * 3000 + normal(1000, 5) + list(3.0 + np.abs(normal(1001, 6))), 7), 100000, [5001]),
    "+inf above the middle, m odd: 0 * inf": (shuffled(normal(2049, 8) + [INF] * 2048, 9), 100000, [4097]),
    "stored NaNs among the taken": ([NAN if i % 7 == 3 else v for i, v in enumerate(normal(4500, 10))], 4400, [4500]),
    "first present cell is a string": ([None, "a"] + normal(4500, 11), 100000, [4502]),
    "all equal": ([2.5] * 4200, 100000, [4200]),
    "a big and a 50-item request in one batch": (normal(5000, 12), 100000, [5000, 50]),
    "more than one workgroup's share of values": ([None if i % 5 == 0 else v for i, v in enumerate(normal(45000, 13))], 40000, [45000, 4097]),
}
CASES["more than one workgroup's share of values"][0][20000] = INF   # (and -0.0 / NaN on the multi-workgroup passes too)
CASES["more than one workgroup's share of values"][0][20001] = -0.0
CASES["more than one workgroup's share of values"][0][20002] = NAN


def backends_of(case):
    vals, top, sizes = CASES[case]
    cfg = single_feature_config({"name": "div_pop", "type": "diversity", "source": "item.popularity", "top": top})
    model = list(cfg["models"])[0]
    orc, hip = OracleBackend(cfg, model), HipBackend(cfg, model)
    for b in (orc, hip):
        for i, v in enumerate(vals):
            if isinstance(v, str):
                b.put_string(f"item=i{i}/div_pop", v)
            elif v is not None:
                b.put_double(f"item=i{i}/div_pop", float(v))
    events = [{"id": f"r{k}", "timestamp": ranklens.TS, "user": None, "session": None, "fields": [], "items": [{"id": f"i{i}"} for i in range(n)]}
              for k, n in enumerate(sizes)]
    return orc, hip, model, events


def batch_matrices(hip, model, events, flat):
    batch = hip.ranker.new_batch()
    batch.load(model, M.RequestSet(events) if flat else events)
    batch.run(None)
    mat = batch.fetch(matrix=True)[2]
    assert (batch.status() == 0).all()
    out = [mat[batch.offsets[r]:batch.offsets[r + 1]].copy() for r in range(len(events))]
    batch.close()
    return out


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_device_median_matches_the_oracle_bit_for_bit(case):
    orc, hip, model, events = backends_of(case)
    try:
        want = [orc.matrix(ev) for ev in events]
        for flat in (False, True):
            got = batch_matrices(hip, model, events, flat)
            for r, (a, b) in enumerate(zip(got, want)):
                assert same(a, b), (case, "flat ids" if flat else "host ids", r)
    finally:
        hip.close()


def profiled_matrix(hip, ev):
    hip.ctx.profile_enable(True)
    mat = hip.matrix(ev)
    return mat, hip.ctx.profile_get("median")[1]


@pytest.mark.gpu
def test_the_median_launches_are_timed_as_median():
    orc, hip, _, events = backends_of("4097 values, m odd")
    try:
        mat, launches = profiled_matrix(hip, events[0])   # through mrk_rank
        assert launches >= 1 and same(mat, orc.matrix(events[0]))
    finally:
        hip.close()


@pytest.mark.gpu
def test_the_host_median_behind_the_switch_gives_the_same_bits():
    _, hip, _, events = backends_of("4097 values, m odd")
    try:
        os.environ["MRK_DIVERSITY_SELECT"] = "0"
        M.reload_switches()
        host, launches = profiled_matrix(hip, events[0])
        assert launches == 0
        os.environ.pop("MRK_DIVERSITY_SELECT")
        M.reload_switches()
        dev, launches = profiled_matrix(hip, events[0])
        assert launches >= 1 and np.array_equal(host.view(np.uint64), dev.view(np.uint64))
    finally:
        os.environ.pop("MRK_DIVERSITY_SELECT", None)
        M.reload_switches()
        hip.close()
