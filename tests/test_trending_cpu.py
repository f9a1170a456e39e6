"""CPU: the host half of the trending recommender (csrc/trending_host.cpp, tests/native/trending_host_test.cpp under ASan +
UBSan), the reference's three known answers (TrendingRecommenderTest.scala:28-72) through the Python restatement the GPU tests
compare with (tests/trending_reference.py), and everything of mrk_trending_* that needs no device: the bitstream (load / id /
predict / save), the config refusals and the null-argument checks."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import trending_reference as T
from metarank_amd import _native
from metarank_amd.trending import HipTrending

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_logic_native_driver(tmp_path):
    exe = str(tmp_path / "trending_host_test")
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(REPO, "tests", "native", "trending_host_test.cpp"), os.path.join(csrc, "trending_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ALL OK" in out.stdout
    assert "interned: p3,p1,p2 now=-10" in out.stdout
    assert "truncations refused: 45 of 45" in out.stdout


@pytest.mark.parametrize("name", sorted(T.KNOWN_ANSWERS))
def test_known_answers_through_the_restatement(name):
    """TrendingRecommenderTest.scala:28-72; the ties p1 / p3 stay in order of first appearance"""
    ids, types, ts, want = T.KNOWN_ANSWERS[name]
    got_ids, got_scores = T.fit(T.TEST_CONFIG, ids, types, ts)
    assert list(zip(got_ids, got_scores.tolist())) == want


def test_restatement_rules():
    day = T.DAY_MS
    now = 10**12
    cfg = {"weights": [{"interaction": "c", "window": "3d", "decay": 2.0}]}
    # rule 3: ts = now - window is outside (strict), one ms later is bucket days - 1; rule 1: a type no weight names moves `now`
    ids, sc = T.fit(cfg, ["a", "b", "z"], ["c", "c", "other"], [now - 3 * day, now - 3 * day + 1, now])
    assert ids == ["b", "a", "z"] and sc.tolist() == [4.0, 0.0, 0.0]
    # rule 3: a bucket outside the array; rule 1: nothing to fit; rule 10: duplicates
    with pytest.raises(T.Refused) as e:
        T.fit({"weights": [{"interaction": "c", "window": "36h"}]}, ["a", "a"], ["c", "c"], [now, now - 30 * 3_600_000])
    assert e.value.status == T.ERR_DIM_MISMATCH
    assert T.fit({"weights": [{"interaction": "c", "window": "36h"}]}, ["a", "a"], ["c", "c"], [now, now - 23 * 3_600_000])[1].tolist() == [2.0]
    with pytest.raises(T.Refused) as e:
        T.fit(cfg, [], [], [])
    assert e.value.status == T.ERR_NOT_FOUND
    with pytest.raises(T.Refused) as e:
        T.fit({"weights": [{"interaction": "c"}, {"interaction": "c"}]}, ["a"], ["c"], [now])
    assert e.value.status == T.ERR_UNSUPPORTED
    # rule 4: every day is visited - 0 * Infinity is NaN - and NaN sorts last; rule 7: +0.0 before -0.0
    ids, sc = T.fit({"weights": [{"interaction": "c", "window": "3d", "decay": 1e200}]}, ["a", "b", "b"], ["c", "c", "c"], [now, now, now - 2 * day])
    assert ids == ["b", "a"] and sc[0] == float("inf") and np.isnan(sc[1])
    ids, sc = T.fit({"weights": [{"interaction": "c", "weight": -1.0, "decay": 0.0, "window": "2d"}]}, ["a", "b", "z"], ["c", "c", "x"], [now - day, now, now])
    assert ids == ["z", "a", "b"] and T.bits(sc).tolist() == T.bits(np.array([0.0, -0.0, -1.0])).tolist()
    # rule 6: no weights at all
    assert T.fit({"weights": []}, ["a", "b"], ["c", "c"], [1, 2])[1].tolist() == [0.0, 0.0]
    # the numpy form the benchmark uses agrees with the scalar loop
    rng = np.random.default_rng(3)
    item = rng.integers(0, 40, 500)
    first = {}
    item = np.array([first.setdefault(int(v), len(first)) for v in item])
    names = ["c", "p", "x"]
    tix = rng.integers(0, 3, 500)
    ts = now - rng.integers(0, 29 * day, 500)
    ts[0] = now
    cfg2 = {"weights": [{"interaction": "p", "weight": 5.0, "decay": 0.5}, {"interaction": "c", "decay": 0.9, "window": "7d"}]}
    ids, sc = T.fit(cfg2, [f"i{v}" for v in item], [names[t] for t in tix], ts.tolist())
    order, score = T.fit_numpy(cfg2, item, tix, names, ts, len(first))
    assert [f"i{v}" for v in order] == ids and T.bits(score[order]).tolist() == T.bits(sc).tolist()


def _model_bytes(items):
    out = struct.pack(">ii", 1, len(items))
    for i, s in items:
        out += struct.pack(">H", len(i)) + i + struct.pack(">d", s)
    return out


def test_bitstream_loads_and_round_trips_without_a_device():
    items = [(b"p2", 3.0), (b"p1", 1.0), ("café".encode(), 1.0), (b"", -0.0), (b"n", float("nan"))]
    data = _model_bytes(items)
    assert data == T.save([i for i, _ in items], [s for _, s in items])
    m = HipTrending.load(data)
    assert m.info() == {"items": 5, "interactions": -1, "now_ms": -1}
    assert m.items() == ["p2", "p1", "café", "", "n"]
    ids, scores = m.predict(2)
    assert ids == ["p2", "p1"] and scores.tolist() == [3.0, 1.0]
    ids, scores = m.predict(50)
    assert len(ids) == 5 and T.bits(scores).tolist() == T.bits(np.array([s for _, s in items])).tolist()
    assert m.save() == data
    L = _native.lib()
    assert L.mrk_trending_id(m.handle, 5) is None and L.mrk_trending_id(m.handle, -1) is None
    n = C.c_int32(9)
    for count in (0, -3):
        assert L.mrk_trending_predict(m.handle, count, None, C.byref(n)) == _native.ERR_INVALID_ARG and n.value == 0
        assert b"count should be greater than 0" in L.mrk_last_error()
    need = C.c_size_t(0)
    small = (C.c_uint8 * 4)()
    assert L.mrk_trending_save(m.handle, small, 4, C.byref(need)) == _native.ERR_INVALID_ARG and need.value == len(data)
    m.close()


def _load_status(data: bytes) -> int:
    h = C.c_void_p()
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    st = _native.lib().mrk_trending_load(None, buf, len(data), C.byref(h))
    assert (st == 0) == bool(h.value)
    if h.value:
        _native.lib().mrk_trending_free(h)
    return st


def test_bitstream_refusals():
    good = _model_bytes([(b"a", 2.0), (b"bb", 1.0)])
    assert _load_status(good) == 0
    assert _load_status(struct.pack(">i", 2) + good[4:]) == _native.ERR_UNSUPPORTED          # "unsupported format 2"
    assert b"unsupported format 2" in _native.lib().mrk_last_error()
    assert _load_status(struct.pack(">ii", 1, 0)) == _native.ERR_PARSE                        # "no items found"
    assert _load_status(struct.pack(">ii", 1, -1) + good[8:]) == _native.ERR_PARSE
    for cut in range(len(good)):
        assert _load_status(good[:cut]) == _native.ERR_PARSE, cut
    assert _load_status(good + b"\0") == _native.ERR_PARSE                                    # trailing garbage
    # writeUTF's limit: 65 535 bytes load and save, one more cannot come from a stream, so it is reached through a fit only
    long_id = _model_bytes([(b"x" * 65535, 1.0)])
    m = HipTrending.load(long_id)
    assert m.save() == long_id
    m.close()


def test_config_refusals_and_null_arguments_without_a_device():
    L = _native.lib()
    out = C.c_void_p()

    def begin(cfg):
        text = cfg if isinstance(cfg, bytes) else json.dumps(cfg).encode()
        st = L.mrk_trending_begin(None, text, C.byref(out))
        assert not out.value
        return st

    assert begin({"weights": [{"interaction": "a"}, {"interaction": "a", "weight": 2.0}]}) == _native.ERR_UNSUPPORTED
    assert b"two weights" in L.mrk_last_error()
    assert begin(b'{"weights":[{"interaction":"a"}') == _native.ERR_PARSE
    assert begin(b"{}") == _native.ERR_PARSE
    assert begin({"weights": [{"interaction": "a", "window": "1w"}]}) == _native.ERR_PARSE
    assert b"duration is in wrong format" in L.mrk_last_error()
    assert begin({"weights": [{"weight": 1.0}]}) == _native.ERR_PARSE
    assert begin({"weights": [{"interaction": "a"}]}) == _native.ERR_INVALID_ARG              # a good config, no context
    assert b"null context" in L.mrk_last_error()
    E = _native.ERR_INVALID_ARG
    assert L.mrk_trending_begin(None, None, C.byref(out)) == E
    assert L.mrk_trending_begin(None, b"{}", None) == E
    assert L.mrk_trending_add(None, None, None, 0, None, None, 0) == E
    assert L.mrk_trending_fit(None, C.byref(out)) == E and L.mrk_trending_fit(None, None) == E
    assert L.mrk_trending_load(None, None, 4, C.byref(out)) == E and L.mrk_trending_load(None, None, 0, None) == E
    assert L.mrk_trending_save(None, None, 0, None) == E
    assert L.mrk_trending_info(None, None, None, None) == E
    assert L.mrk_trending_id(None, 0) is None
    n = C.c_int32(3)
    assert L.mrk_trending_predict(None, 1, None, C.byref(n)) == E and n.value == 0
    assert L.mrk_trending_predict(None, 1, None, None) == E
    L.mrk_trending_builder_free(None)
    L.mrk_trending_free(None)
    assert L.mrk_abi_version() == 9 and L.mrk_abi_layout(None, 0) == 33   # new symbols only
