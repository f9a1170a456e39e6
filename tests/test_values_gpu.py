"""GPU: mrk_values / values batches (TrainBuffer.handleRanking's ItemValue.fromState in ValueMode.OfflineTraining) against the
oracle's online matrix with the `position` columns rewritten (tests/values_reference.py), bit for bit, in every launch shape:
the one-launch values kernel (interpreting and specialised, with and without op split), the workgroup-per-request kernel in
its plain, op-split and sliced forms, the item-parallel kernels, and the stand-alone path of requests over 1 024 items."""
import contextlib
import os

import numpy as np
import pytest

import metarank_amd as M
from metarank_amd import _native
import values_reference as R
from backends import HipBackend, single_feature_config, ranking_event
from workloads import ranklens

pytestmark = pytest.mark.gpu

N_ITEMS, N_SESS = 300, 40
SWITCHES = ("MRK_RANK_JIT", "MRK_RANK_FUSED", "MRK_FUSED_SPLIT", "MRK_FUSED_SLICES", "MRK_FUSED_THREADS", "MRK_VALUES_ONE")


@contextlib.contextmanager
def switches(**kw):
    """the library's experiment switches for the duration of the block (read once: reload after every change)"""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in kw.items()})
        M.reload_switches()
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        M.reload_switches()


def config():
    """the stock Ranklens mapping (position: 5 among its item features) plus a ranking feature defined LAST: it is emitted first"""
    cfg = ranklens.ranklens_config()
    cfg["features"].append({"name": "hour", "type": "local_time", "source": "ranking.timestamp", "parse": "time_of_day"})
    return R.with_emission_model(cfg)


@pytest.fixture(scope="module")
def env(ctx):
    """the oracle and the library over the same few hundred items; the interpreting kernels unless a test says otherwise
    (a specialised kernel is a compile of its own: the tests that cover those name them)"""
    cfg = config()
    orc = R.ValuesOracle(cfg)
    hip = HipBackend(cfg, R.EMISSION_MODEL, ctx)
    for be in (orc.backend, hip):
        ranklens.load_state(be, ranklens.generate_state(N_ITEMS, N_SESS))
    with switches(MRK_RANK_JIT=0):
        yield cfg, orc, hip
    hip.close()


def requests(sizes, seed):
    out = []
    for k, n in enumerate(sizes):
        ev = ranklens.generate_requests(1, n, N_ITEMS, N_SESS, seed=seed + k, unknown_frac=0.05)[0]
        ev["id"] = f"req{k}"
        out.append(ev)
    return out


def expected(orc, reqs, offline=True):
    return np.concatenate([orc.expected(ev, offline) for ev in reqs])


def run_batch(hip, reqs, model=None, offline=True):
    batch = hip.ranker.new_batch()
    try:
        batch.load_values(reqs, model=model, offline=offline)
        batch.run(None)
        scores, order, mat = batch.fetch(matrix=True)
        status = batch.status()
        offsets = batch.offsets
    finally:
        batch.close()
    assert not status.any() and not scores.any()
    for r in range(len(reqs)):   # NoopRanker: every request in its own order
        assert order[offsets[r]:offsets[r + 1]].tolist() == list(range(offsets[r + 1] - offsets[r]))
    return mat


def launches(ctx, name):
    return ctx.profile_get(name)[1]


def test_known_answer_position(ctx):
    """PositionFeatureTest.scala:14-31: position 5, three items - online [5, 5, 5], offline [0, 1, 2]"""
    hip = HipBackend(single_feature_config({"name": "pos", "type": "position", "position": 5}), "random", ctx)
    try:
        ev = ranking_event(["p1", "p2", "p3"])
        for model in (None, "random"):
            assert hip.ranker.values(ev, model=model, offline=True)[:, 0].tolist() == [0.0, 1.0, 2.0]
            assert hip.ranker.values(ev, model=model, offline=False)[:, 0].tolist() == [5.0, 5.0, 5.0]
        assert hip.ranker.values_columns() == [("pos", 0, 1, "single")] and hip.ranker.values_dim() == 1
    finally:
        hip.close()


def test_columns_and_dim_of_the_loaded_config(env):
    cfg, orc, hip = env
    cols = hip.ranker.values_columns()
    assert [c[0] for c in cols] == R.emission_order(cfg["features"]) and cols[0] == ("hour", 0, 1, "single")
    assert {c[0]: (c[1], c[2]) for c in cols} == orc.offsets
    assert hip.ranker.values_dim() == orc.dim == cols[-1][1] + cols[-1][2]
    assert dict((c[0], c[3]) for c in cols)["genre"] == "category"
    with pytest.raises(M.MrkError) as e:
        hip.ranker.values_dim("nope")
    assert e.value.status == _native.ERR_NOT_FOUND and "model nope is not configured" in e.value.message
    with pytest.raises(M.MrkError) as e:
        hip.ranker.values(requests([3], 5)[0], model="nope")
    assert e.value.status == _native.ERR_NOT_FOUND


@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_one_request(env, n):
    """mrk_values, the mapping program: 65 crosses a wavefront, 130 the 128 lanes of a two-wavefront workgroup"""
    cfg, orc, hip = env
    ev = requests([n], 100 + n)[0]
    hip.ranker.ctx.profile_enable(True)
    try:
        before = launches(hip.ranker.ctx, "rank_values"), launches(hip.ranker.ctx, "assemble")
        got = hip.ranker.values(ev)
        assert R.same_bits(got, orc.expected(ev))
        pos = orc.offsets["position"][0]
        assert got[:, pos].tolist() == [float(i) for i in range(n)]
        # ONE launch, and not the assembly kernel's
        assert (launches(hip.ranker.ctx, "rank_values"), launches(hip.ranker.ctx, "assemble")) == (before[0] + 1, before[1])
        online = hip.ranker.values(ev, offline=False)
        assert R.same_bits(online, orc.expected(ev, offline=False)) and set(online[:, pos].tolist()) == {5.0}
        # ... which is what mrk_rank(model = NULL, out_matrix) of a model that lists the mapping in emission order assembles
        assert R.same_bits(online, hip.ranker.rerank(R.EMISSION_MODEL, ev, None, explain=True)[0])
    finally:
        hip.ranker.ctx.profile_enable(False)


@pytest.mark.parametrize("sizes", [[5, 64, 70], [1] * 70], ids=["5-64-70", "70x1"])
def test_batches_restart_the_index_per_request(env, sizes):
    cfg, orc, hip = env
    reqs = requests(sizes, 300)
    want = expected(orc, reqs)
    pos = orc.offsets["position"][0]
    assert want[:, pos].tolist() == [float(i) for n in sizes for i in range(n)]
    assert R.same_bits(run_batch(hip, reqs), want)
    # the item-parallel kernels: lanes of one wavefront belong to different requests (70 one-item requests: all of them do)
    with switches(MRK_RANK_JIT=0, MRK_RANK_FUSED=0):
        assert R.same_bits(run_batch(hip, reqs), want)


def test_large_request_takes_the_stand_alone_path(env):
    """1 100 items: more than a workgroup's request (not fused_ok) - pre-pass launch, item-parallel assembly, a copy"""
    cfg, orc, hip = env
    reqs = requests([1100, 3], 400)
    want = expected(orc, reqs)
    hip.ranker.ctx.profile_enable(True)
    try:
        before = launches(hip.ranker.ctx, "rank_values")
        assert R.same_bits(run_batch(hip, reqs), want)
        assert launches(hip.ranker.ctx, "rank_values") == before
        assert R.same_bits(hip.ranker.values(reqs[0]), want[:1100])
    finally:
        hip.ranker.ctx.profile_enable(False)
    pos = orc.offsets["position"][0]
    assert want[1099, pos] == 1099.0 and want[1100:, pos].tolist() == [0.0, 1.0, 2.0]


VARIANTS = [
    dict(MRK_RANK_JIT=0),                                            # the one-launch values kernel, interpreting, op split by batch shape (4)
    dict(MRK_RANK_JIT=0, MRK_FUSED_SPLIT=1),
    dict(MRK_RANK_JIT=0, MRK_FUSED_SPLIT=2),
    dict(MRK_RANK_JIT="require"),                                    # ... specialised (hiprtc), op split 4
    dict(MRK_RANK_JIT="require", MRK_FUSED_SPLIT=1),
    dict(MRK_RANK_JIT=0, MRK_VALUES_ONE=0),                          # launches + copy: the workgroup-per-request kernel, op split 4
    dict(MRK_RANK_JIT=0, MRK_VALUES_ONE=0, MRK_FUSED_SPLIT=1),
    dict(MRK_RANK_JIT=0, MRK_VALUES_ONE=0, MRK_FUSED_SPLIT=2),
    dict(MRK_RANK_JIT=0, MRK_FUSED_THREADS=64, MRK_FUSED_SLICES=2, MRK_FUSED_SPLIT=1),   # sliced: two workgroups per request (never the one-launch kernel)
    dict(MRK_RANK_JIT="require", MRK_VALUES_ONE=0, MRK_FUSED_SPLIT=1),                   # the specialised matrix kernel, without a model
    dict(MRK_RANK_JIT=0, MRK_RANK_FUSED=0),                          # pre-pass launch + item-parallel assembly
]


def test_kernel_variants_give_identical_bytes(env):
    cfg, orc, hip = env
    reqs = requests([5, 64, 70], 300)
    want = expected(orc, reqs)
    hip.ranker.ctx.profile_enable(True)
    try:
        for v in VARIANTS:
            with switches(**v):
                before = launches(hip.ranker.ctx, "rank_values")
                got = run_batch(hip, reqs)
                one = launches(hip.ranker.ctx, "rank_values") - before
            assert R.same_bits(got, want), v
            takes_one = str(v.get("MRK_VALUES_ONE", 1)) != "0" and str(v.get("MRK_RANK_FUSED", 1)) != "0" and "MRK_FUSED_SLICES" not in v
            assert one == (1 if takes_one else 0), v
    finally:
        hip.ranker.ctx.profile_enable(False)


def test_model_program_keeps_descriptor_order(env):
    """a model's program: offline it differs from mrk_rank's matrix in the position column only; online it IS that matrix"""
    cfg, orc, hip = env
    model = "xgboost"
    morc = R.ValuesOracle(cfg, model)
    ranklens.load_state(morc.backend, ranklens.generate_state(N_ITEMS, N_SESS))
    assert [c[0] for c in hip.ranker.values_columns(model)] == [n for n in cfg["models"][model]["features"]]
    assert hip.ranker.values_dim(model) == hip.ranker.dim(model) == morc.dim
    reqs = requests([5, 64, 70], 500)
    for ev in reqs:
        ranked = hip.ranker.rerank(model, ev, None, explain=True)[0]
        assert R.same_bits(hip.ranker.values(ev, model=model, offline=False), ranked)
        assert R.same_bits(ranked, morc.expected(ev, offline=False))
        assert R.same_bits(hip.ranker.values(ev, model=model, offline=True), morc.expected(ev, offline=True))
    assert R.same_bits(run_batch(hip, reqs, model=model), np.concatenate([morc.expected(ev) for ev in reqs]))
    assert R.same_bits(run_batch(hip, reqs, model=model, offline=False), np.concatenate([morc.expected(ev, False) for ev in reqs]))


def test_values_binary_decodes_like_rank_binary(env):
    """RankingEventFormat input through mrk_rank_binary's decoder"""
    import ctypes as C

    from oracle import codec

    cfg, orc, hip = env
    ev = requests([7], 600)[0]
    blob = codec.ranking_event(ev)
    n = C.c_int(0)
    mat = np.empty((16, orc.dim), dtype=np.float64)
    _native.check(_native.lib().mrk_values_binary(hip.ranker.ctx.handle, None, 1, blob, len(blob), C.byref(n), mat.ctypes.data_as(C.c_void_p), 16))
    assert n.value == 7 and R.same_bits(mat[:7], orc.expected(ev))
