"""CPU: the `position_bias` key of the train config through mrk_train_begin (its defaults, every refusal with its status, both backends),
and the host half of step 3b under ASan + UBSan (tests/native/train_bias_host_test.cpp: decoder, cost table, update of the factors)."""
import ctypes as C
import json
import os
import subprocess

import pytest

from metarank_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD, PARSE, RANGE, UNSUPPORTED = "good", _native.ERR_PARSE, _native.ERR_INVALID_ARG, _native.ERR_UNSUPPORTED


def test_host_logic_native_driver(tmp_path):
    exe = str(tmp_path / "train_bias_host_test")
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(REPO, "tests", "native", "train_bias_host_test.cpp"), os.path.join(csrc, "train_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("backend", ["lightgbm", "xgboost"])
@pytest.mark.parametrize("value,want", [
    (None, GOOD), ({}, GOOD), ({"positions": None, "norm": None}, GOOD), ({"positions": 1}, GOOD), ({"positions": 4096, "norm": 0}, GOOD),
    (True, PARSE), ([8], PARSE), ({"positions": "8"}, PARSE), ({"positions": 2.5}, PARSE), ({"norm": "1"}, PARSE), ({"position": 8}, PARSE),
    ({"positions": 0}, RANGE), ({"positions": 4097}, RANGE), ({"norm": -1}, RANGE)])
def test_the_position_bias_key(backend, value, want):
    L = _native.lib()
    out = C.c_void_p()
    st = L.mrk_train_begin(None, json.dumps({"backend": backend, "position_bias": value}).encode(), C.byref(out))
    assert not out.value
    if want == GOOD:                                          # a config that parses ends at the missing context
        assert st == _native.ERR_INVALID_ARG and b"null context" in L.mrk_last_error()
    else:
        assert st == want and b"position" in L.mrk_last_error()
    assert L.mrk_train_begin(None, json.dumps({"backend": backend, "debias": True, "position_bias": value}).encode(), C.byref(out)) == (
        UNSUPPORTED if want == GOOD else want)
    if want == GOOD:
        assert b"use position_bias" in L.mrk_last_error()
