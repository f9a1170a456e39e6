"""CPU: the host half of the semantic fit (mrk_index_build_texts): the piece planner knn_plan_pieces of csrc/index_host.cpp
under ASan + UBSan as a stand-alone program (tests/native/semantic_plan_test.cpp), and the argument checks of the two new
exports that need no device."""
import ctypes as C
import os
import subprocess

from metarank_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_piece_planner_native_driver(tmp_path):
    exe = str(tmp_path / "semantic_plan_test")
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(REPO, "tests", "native", "semantic_plan_test.cpp"), os.path.join(csrc, "index_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ALL OK" in out.stdout


def test_null_arguments_are_refused_without_a_device():
    L = _native.lib()
    E = _native.ERR_INVALID_ARG
    out = C.c_void_p(1)
    assert L.mrk_index_build_texts(None, None, None, None, 1, 0, C.byref(out)) == E and not out.value
    assert b"null context" in L.mrk_last_error()
    assert L.mrk_index_build_texts(None, None, None, None, 0, 0, None) == E
    assert b"out is null" in L.mrk_last_error()
    assert L.mrk_index_vectors(None, None, 1, None) == E
    assert b"null index" in L.mrk_last_error()
    assert L.mrk_abi_version() == 9 and L.mrk_abi_layout(None, 0) == 33   # new symbols only


def test_fp16_bound_holds_for_the_catalogue_on_the_oracle():
    """the GPU test holds an fp16 handle's rows to a cosine within 3e-3 of the f32 handle's (test_encoder_gpu.py's ATOL_COS): the
    chosen 150 texts keep that bound in the numpy graph (fp16 rounding points against fp32) with a wide margin"""
    import numpy as np
    from safetensors.numpy import load_file

    import semantic_cases as S
    from metarank_amd.encoder import HipTokenizer
    from oracle import bert

    ids, texts = S.catalogue()
    assert len(texts) == 150 and len(set(ids)) == 150 and texts[5] == ""
    tok = HipTokenizer(open(os.path.join(S.GOLDEN, "tokenizer_tiny.json"), "rb").read())
    i, t, m = tok.encode_batch(texts)
    lens = m.sum(axis=1)
    assert lens.min() == 2 and lens.max() == 24 and lens[5] == 2 and lens[70] == 24 and len(set(lens.tolist())) > 15
    w = bert.strip_prefix(load_file(os.path.join(S.GOLDEN, "encoder_tiny.safetensors")))
    a, b = bert.embed(w, i, t, m, heads=2), bert.embed(w, i, t, m, heads=2, fp16=True)
    cos = (a * b).sum(axis=1) / np.sqrt((a * a).sum(axis=1) * (b * b).sum(axis=1))
    assert np.abs(cos - 1.0).max() < 3e-3 / 100
