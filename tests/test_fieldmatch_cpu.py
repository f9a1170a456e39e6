"""CPU: field_match term / ngram / bm25 on the device, everything that needs no device - the Python transcription the GPU tests
compare with (tests/fieldmatch_reference.py) pinned on the reference's own known answers, the host half (csrc/match_host.cpp,
tests/native/match_host_test.cpp under ASan + UBSan), and the program the config builds with and without "match": "device"."""
import ctypes as C
import json
import os
import random
import re
import struct
import subprocess

import fieldmatch_reference as R
from metarank_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what tests/native/match_host_test.cpp parses (kDic) and prints idf * w for
NATIVE_DIC = {"docs": 1000, "avgdl": 7.25, "termfreq": {"common": 900, "rare": 3, "mid": 120, "over": 1500, "zero": 0, "café": 17}}


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_reference_known_answers_term_and_ngram():
    # FieldMatchFeatureTest.scala:57-64: query "foo" against the 3-grams of "foobar"
    assert R.match_score(["foo"], ["bar", "foo", "oba", "oob"]) == 0.25
    # NgramMatcherTest.scala:20-30 / TermMatcherTest.scala
    assert R.match_score(["a", "b", "c"], ["a", "b", "c"]) == 1.0
    assert R.match_score(["a"], ["a", "b"]) == 0.5
    assert R.match_score(["c", "d"], ["a", "b"]) == 0.0
    assert R.match_score([], ["a"]) == 0.0 and R.match_score(["a"], []) == 0.0
    # NgramMatcherTest.scala:10-18 (whitespace analyzer: the split is the test's)
    assert R.ngram_tokenize("fooba foo".split(), 3) == ["foo", "oba", "oob"]
    assert R.ngram_tokenize("foobar".split(), 3) == ["bar", "foo", "oba", "oob"]
    assert R.term_tokenize(["hamster", "greet", "greet"]) == ["greet", "hamster"] and R.term_tokenize([]) == []
    assert R.column("term", None, [["a"]]) == [0.0] and R.column("term", ["a"], [None, ["a"]]) == [0.0, 1.0]


def test_reference_known_answers_bm25():
    dic = {"docs": 3, "avgdl": 3.0, "termfreq": {"foo": 1, "bar": 2, "baz": 3}}   # BM25MatcherTest.scala
    assert abs(R.bm25_score(["baz"], ["bar", "baz"], dic) - 0.15) <= 0.01
    assert abs(R.bm25_score(["foo"], ["foo"], dic) - 1.34) <= 0.01
    assert R.bm25_score([], ["foo"], dic) == 0.0 and bits(R.bm25_score(["foo"], [], dic)) == 0
    # gtf > docs: a negative idf, a negative score
    assert R.bm25_score(["x"], ["x"], {"docs": 3, "avgdl": 3.0, "termfreq": {"x": 10}}) < 0.0


def test_string_order_is_utf16():
    assert R.compare_to("�", "\U0001f600") > 0 and "�".encode() < "\U0001f600".encode()   # UTF-8 says the opposite
    assert R.compare_to("ab", "abc") < 0 and R.compare_to("b", "a") > 0 and R.compare_to("x", "x") == 0
    assert R.unique(["�", "b", "\U0001f600", "b"]) == ["b", "\U0001f600", "�"]
    assert R.strictly_ascending(["a", "\U0001f600", "�"]) and not R.strictly_ascending(["a", "a"])


def test_merge_walk_equals_the_set_formula():
    rng = random.Random(11)
    alphabet = [chr(c) for c in range(ord("a"), ord("k"))] + ["é", "�", "\U0001f600", ""]
    for _ in range(400):
        vocab = {"".join(rng.choice(alphabet) for _ in range(rng.randint(1, 3))) for _ in range(rng.randint(1, 30))}
        vocab = sorted(vocab, key=R.utf16_key)
        q = [t for t in vocab if rng.random() < 0.5]
        d = [t for t in vocab if rng.random() < 0.5]
        assert R.strictly_ascending(q) and R.strictly_ascending(d)
        inter = len(set(q) & set(d))
        want = 0.0 if not q or not d else inter / (len(q) + len(d) - inter)
        assert bits(R.match_score(q, d)) == bits(want)


def test_host_logic_native_driver(tmp_path):
    exe = str(tmp_path / "match_host_test")
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(REPO, "tests", "native", "match_host_test.cpp"), os.path.join(csrc, "match_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ALL OK" in out.stdout
    got = dict(re.findall(r"^idfw (\S+) ([0-9a-f]{16})$", out.stdout, flags=re.M))
    assert set(got) == set(NATIVE_DIC["termfreq"]) | {"absent"}
    for term, hexbits in got.items():
        want = R.bm25_idf(NATIVE_DIC["docs"], NATIVE_DIC["termfreq"].get(term, 0)) * (1 * (R.K1 + 1.0))
        assert int(hexbits, 16) == bits(want), term


def _config(match: bool):
    def fm(name, field, method):
        f = {"name": name, "type": "field_match", "rankingField": "ranking.query", "itemField": "item." + field, "method": method}
        if match:
            f["match"] = "device"
        return f
    feats = [{"name": "pop", "type": "number", "scope": "item", "source": "item.pop"},
             fm("m_term", "title", {"type": "term", "language": "en"}),
             fm("m_ngram", "desc", {"type": "ngram", "language": "en", "n": 3}),
             fm("m_bm25", "tags", {"type": "bm25", "language": "en", "termFreq": "/data/tf.json"})]
    return {"features": feats, "models": {"xgboost": {"type": "lambdamart", "features": [f["name"] for f in feats]}}}


def _specialize(cfg):
    lib = _native.lib()
    js = json.dumps(cfg).encode()
    need = C.c_size_t(0)
    rc = lib.mrk_config_specialize(js, len(js), b"xgboost", 1, 0, None, 0, C.byref(need))
    if rc == _native.ERR_INVALID_ARG and need.value:
        buf = (C.c_uint8 * need.value)()
        rc = lib.mrk_config_specialize(js, len(js), b"xgboost", 1, 0, buf, need.value, C.byref(need))
        return rc, bytes(buf[:need.value]).decode()
    return rc, ""


def _op_rows(text):
    body = text[text.index("struct JitOps"):text.index("struct JitPrep")]
    return re.findall(r"\{(\d+),(\d+),(\d+),(\d+),\{(-?\d+),(\d+)\},.*?,(\d+),(\d+),\d+,\d+,[^}]*\},", body)


def test_program_with_and_without_the_opt_in():
    """through the C ABI, no device (mrk_config_specialize builds the program on the host and returns it as constants)"""
    OP_SCALAR_DOUBLE, OP_FILL_NAN, OP_FIELD_MATCH, SC_ITEM = 0, 12, 14, 1
    rc, text = _specialize(_config(True))
    assert rc == 0, _native.lib().mrk_last_error()
    rows = [tuple(int(x) for x in r) for r in _op_rows(text)]
    assert [r[0] for r in rows] == [OP_SCALAR_DOUBLE, OP_FIELD_MATCH, OP_FIELD_MATCH, OP_FIELD_MATCH]
    assert [r[1] for r in rows] == [0, 1, 2, 3] and all(r[2] == 1 and r[3] == SC_ITEM for r in rows)
    # every match feature reads a declared item column of its own (tag index >= 0, distinct value cells)
    assert all(r[4] >= 0 for r in rows) and len({r[5] for r in rows}) == 4
    # const blocks: term / ngram 2 + 128 doubles, bm25 3 + 64 + 64; i1 = 1 marks bm25
    assert [(r[6], r[7]) for r in rows[1:]] == [(0, 0), (130, 0), (260, 1)]
    assert "n_ops = 4, n_prep = 0, dim = 4, n_consts = 391" in text
    # without the key: host-computed columns, exactly as before - NaN fill, no column, no constants
    rc, text0 = _specialize(_config(False))
    assert rc == 0
    rows0 = [tuple(int(x) for x in r) for r in _op_rows(text0)]
    assert [r[0] for r in rows0] == [OP_SCALAR_DOUBLE, OP_FILL_NAN, OP_FILL_NAN, OP_FILL_NAN]
    assert all(r[4] == -1 and r[5] == 0 and r[6] == 0 and r[7] == 0 for r in rows0[1:])
    assert "n_ops = 4, n_prep = 0, dim = 4, n_consts = 0, item_fixed = 16" in text0
    # the opt-in accepts the three token matchers only, and only the value "device"
    for method in ({"type": "bi-encoder", "dim": 8}, {"type": "cross-encoder"}, {"type": "fuzzy"}, {}):
        cfg = _config(True)
        cfg["features"][1]["method"] = method
        assert _specialize(cfg)[0] == _native.ERR_PARSE
    cfg = _config(True)
    cfg["features"][1]["match"] = "host"
    assert _specialize(cfg)[0] == _native.ERR_PARSE
    cfg = _config(True)
    del cfg["features"][1]["itemField"]
    assert _specialize(cfg)[0] == _native.ERR_PARSE


def test_new_symbol_and_limits_are_in_the_header():
    L = _native.lib()
    hdr = open(os.path.join(REPO, "include", "mrk.h")).read()
    assert re.search(r"\bint mrk_config_bind_termfreq\(mrk_ctx \*ctx, const char \*feature, const char \*json_bytes, size_t len\);", hdr)
    assert re.search(r"#define MRK_MATCH_MAX_QUERY_TOKENS 128\b", hdr) and re.search(r"#define MRK_MATCH_MAX_QUERY_TOKENS_BM25 64\b", hdr)
    assert hasattr(L, "mrk_config_bind_termfreq") and "mrk_config_bind_termfreq" in _native.SIGNATURES
    assert L.mrk_config_bind_termfreq(None, b"f", b"{}", 2) == _native.ERR_INVALID_ARG
    assert b"null argument" in L.mrk_last_error()
    assert L.mrk_abi_version() == 9 and L.mrk_abi_layout(None, 0) == 33   # additive


def test_request_marshals_an_empty_query_as_a_string_list():
    """An empty Python list has no element type; under "__tokens:<name>" it is the empty STRING list the library expects (an
    empty query, not the absent-field path).  Any other name keeps the number-list reading."""
    from metarank_amd.request import F_NUMBER_LIST, F_STRING_LIST, Request

    rq = Request({"id": "r", "fields": [{"name": "__tokens:m", "value": []}, {"name": "other", "value": []},
                                        {"name": "__tokens:n", "value": ["a", "b"]}], "items": ["i"]})
    got = [(rq.c.fields[i].type, rq.c.fields[i].n) for i in range(3)]
    assert got == [(F_STRING_LIST, 0), (F_NUMBER_LIST, 0), (F_STRING_LIST, 2)]
    assert bool(rq.c.fields[0].strs)   # n == 0 with a valid pointer
