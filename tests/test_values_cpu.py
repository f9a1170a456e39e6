"""CPU: the values programs (TrainBuffer.handleRanking's ItemValue.fromState) as far as no device is needed - the mapping
program's column order, the columns text, the item-index op in offline programs only, and the unchanged ABI.  What the
programs compute is a GPU test (tests/test_values_gpu.py)."""
import ctypes as C
import json
import re

import values_reference as R
from metarank_amd import _native
from workloads import ranklens

# `position`, `local_time` and a `string index` feature OUT of emission order: an item feature, then a ranking feature, ...
FEATURES = [
    {"name": "pos", "type": "position", "position": 5},
    {"name": "popularity", "type": "number", "scope": "item", "source": "metadata.popularity"},
    {"name": "hour", "type": "local_time", "source": "ranking.timestamp", "parse": "time_of_day"},
    {"name": "genre", "type": "string", "scope": "item", "source": "metadata.genres", "encode": "index", "values": ["a", "b", "c"]},
    {"name": "tags", "type": "string", "scope": "item", "source": "metadata.tags", "encode": "onehot", "values": ["x", "y", "z", "w"]},
    {"name": "agent", "type": "ua", "field": "platform", "source": "ranking.ua", "dim": 3},
    {"name": "clicks", "type": "window_count", "interaction": "click", "scope": "item", "bucket": "24h", "periods": [7, 30]},
    {"name": "noise", "type": "random"},
]
CONFIG = {"features": FEATURES, "models": {"m": {"type": "lambdamart", "features": ["popularity", "pos", "genre"]},
                                           "plain": {"type": "lambdamart", "features": ["popularity", "genre"]}}}


def columns(cfg, model):
    lib = _native.lib()
    js = json.dumps(cfg).encode()
    need = C.c_size_t(0)
    rc = lib.mrk_config_values_columns(js, len(js), model, None, 0, C.byref(need))
    if rc != _native.ERR_INVALID_ARG or not need.value:
        return rc, ""
    buf = C.create_string_buffer(need.value)
    rc = lib.mrk_config_values_columns(js, len(js), model, buf, need.value, C.byref(need))
    return rc, buf.value.decode()


def specialize_values(cfg, model, mode, what):
    lib = _native.lib()
    js = json.dumps(cfg).encode()
    need = C.c_size_t(0)
    rc = lib.mrk_config_specialize_values(js, len(js), model, mode, what, None, 0, C.byref(need))
    if rc == _native.ERR_INVALID_ARG and need.value:
        buf = (C.c_uint8 * need.value)()
        rc = lib.mrk_config_specialize_values(js, len(js), model, mode, what, buf, need.value, C.byref(need))
        return rc, bytes(buf[:need.value]).decode()
    return rc, ""


def op_kinds(text):
    rows = re.search(r"struct JitOps \{.*?= \{(.*?)\};\n", text, re.S).group(1)
    return [int(k) for k in re.findall(r"^\s*\{(\d+),", rows, re.M)]


def test_mapping_columns_come_in_emission_order():
    rc, text = columns(CONFIG, None)
    assert rc == 0, _native.lib().mrk_last_error()
    # the RankingFeatures (local_time, ua) in `features:` order, then the ItemFeatures in `features:` order; ua / random are
    # host-supplied "__ext:" columns with their dim; CategoryValue for string encode: index, VectorValue for the list-valued ones
    assert text == ("hour\t0\t1\tsingle\n" "agent\t1\t3\tvector\n" "pos\t4\t1\tsingle\n" "popularity\t5\t1\tsingle\n" "genre\t6\t1\tcategory\n"
                    "tags\t7\t4\tvector\n" "clicks\t11\t2\tvector\n" "noise\t13\t1\tsingle\n")
    assert [ln.split("\t")[0] for ln in text.splitlines()] == R.emission_order(FEATURES)


def test_values_dim_is_the_sum_of_the_columns():
    for model, want in ((None, 14), (b"m", 3), (b"plain", 2)):
        rc, text = columns(CONFIG, model)
        rows = [ln.split("\t") for ln in text.splitlines()]
        assert rc == 0 and int(rows[-1][1]) + int(rows[-1][2]) == want
    # the stock Ranklens mapping: every feature is an item feature, so its rows are the stock model's (which lists them all, in order)
    cfg = ranklens.ranklens_config()
    rc, text = columns(cfg, None)
    rc2, text2 = columns(cfg, b"xgboost")
    assert rc == 0 and rc2 == 0 and len(text.splitlines()) == len(cfg["features"])
    if cfg["models"]["xgboost"]["features"] == [f["name"] for f in cfg["features"]]:
        assert text == text2


def test_model_program_keeps_descriptor_order():
    rc, text = columns(CONFIG, b"m")
    assert rc == 0 and text == "popularity\t0\t1\tsingle\npos\t1\t1\tsingle\ngenre\t2\t1\tcategory\n"


def test_unknown_model_is_the_existing_error():
    lib = _native.lib()
    rc, _ = columns(CONFIG, b"nope")
    assert rc == _native.ERR_NOT_FOUND and b"model nope is not configured" in lib.mrk_last_error()
    js = json.dumps(CONFIG).encode()
    need = C.c_size_t(0)
    assert lib.mrk_config_specialize(js, len(js), b"nope", 1, 0, None, 0, C.byref(need)) == _native.ERR_NOT_FOUND   # the same status and text
    assert b"model nope is not configured" in lib.mrk_last_error()
    assert specialize_values(CONFIG, b"nope", 1, 0)[0] == _native.ERR_NOT_FOUND
    assert specialize_values(CONFIG, None, 2, 0)[0] == _native.ERR_INVALID_ARG   # mode is 0 | 1
    # argument checks of the context-bound calls come before any device work
    assert lib.mrk_values(None, None, 1, None, None) == _native.ERR_INVALID_ARG
    assert lib.mrk_values_dim(None, None) == _native.ERR_INVALID_ARG
    assert lib.mrk_values_columns(None, None, None, 0, C.byref(need)) == _native.ERR_INVALID_ARG
    assert lib.mrk_batch_load_values(None, None, 1, None, 0, None) == _native.ERR_INVALID_ARG
    n = C.c_int(-1)
    assert lib.mrk_values_binary(None, None, 1, None, 0, C.byref(n), None, 0) == _native.ERR_INVALID_ARG and n.value == 0


def test_only_offline_programs_with_a_position_hold_the_item_index_op():
    OP_CONST, OP_ITEM_INDEX = 11, 15
    for model in (None, b"m"):
        rc, off = specialize_values(CONFIG, model, 1, 0)
        rc2, on = specialize_values(CONFIG, model, 0, 0)
        assert rc == 0 and rc2 == 0, _native.lib().mrk_last_error()
        k_off, k_on = op_kinds(off), op_kinds(on)
        assert k_off.count(OP_ITEM_INDEX) == 1 and OP_ITEM_INDEX not in k_on
        # ... in the place of the online program's constant, and nowhere else do the two differ
        at = k_off.index(OP_ITEM_INDEX)
        assert k_on[at] == OP_CONST and k_off[:at] + k_off[at + 1:] == k_on[:at] + k_on[at + 1:]
        # the offline program needs one request constant fewer: position is no longer one
        n_consts = lambda t: int(re.search(r"n_consts = (\d+)", t).group(1))
        assert n_consts(off) == n_consts(on) - 1
    # a program without `position` is the same program in both modes - text and all: its kernels are shared with mrk_rank's
    rc, off = specialize_values(CONFIG, b"plain", 1, 0)
    rc2, on = specialize_values(CONFIG, b"plain", 0, 0)
    assert rc == 0 and rc2 == 0 and off == on and OP_ITEM_INDEX not in op_kinds(off)
    # the online program of a model IS the program mrk_config_specialize shows
    js = json.dumps(CONFIG).encode()
    need = C.c_size_t(0)
    lib = _native.lib()
    lib.mrk_config_specialize(js, len(js), b"m", 1, 0, None, 0, C.byref(need))
    buf = (C.c_uint8 * need.value)()
    assert lib.mrk_config_specialize(js, len(js), b"m", 1, 0, buf, need.value, C.byref(need)) == 0
    assert bytes(buf[:need.value]).decode() == specialize_values(CONFIG, b"m", 0, 0)[1]


def test_the_one_launch_values_kernel_is_a_translation_unit_of_its_own():
    rc, src = specialize_values(CONFIG, None, 1, 0 | (12 << 8))
    flat = src.replace("\n", "")
    assert rc == 0 and "mrk_jit_rank_values(" in flat and "rank_values_body<true>" in flat and "mrk_jit_rank_matrix(" not in flat
    rc, src = specialize_values(CONFIG, None, 1, 0 | (3 << 8))
    assert rc == 0 and "mrk_jit_rank_matrix(" in src.replace("\n", "") and "mrk_jit_rank_values(" not in src.replace("\n", "")
    assert specialize_values(CONFIG, None, 1, 0 | (13 << 8))[0] == _native.ERR_INVALID_ARG


def test_abi_is_unchanged():
    lib = _native.lib()
    assert lib.mrk_abi_version() == 9
    assert lib.mrk_abi_layout(None, 0) == 33
