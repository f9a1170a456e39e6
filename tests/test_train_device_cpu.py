"""CPU: step 2d of the LambdaMART fit (include/mrk.h: the trainer's matrix from device memory) as far as it needs no device - the cut
rule the device's bin finder calls (csrc/train_host.hpp train_cut_at; tests/native/train_cuts_test.cpp under ASan + UBSan, against
train_bin_bounds / train_bin_bounds_f32 on the unsorted cells, bit for bit) and the argument errors of mrk_train_append_device,
mrk_train_seal and mrk_train_bounds that are judged before any device work.  A trainer cannot exist without a device, so `which` is
judged before the trainer here; what needs a live trainer (mrk_train_bounds before any set among it) is tests/test_train_device_gpu.py's."""
import ctypes as C
import os
import re
import subprocess

from metarank_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cut_rule_native_driver(tmp_path):
    exe = str(tmp_path / "train_cuts_test")
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(REPO, "tests", "native", "train_cuts_test.cpp"), os.path.join(csrc, "train_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ALL OK" in out.stdout
    assert int(re.search(r"(\d+) comparisons", out.stdout).group(1)) >= 500


def test_argument_errors_without_a_device():
    L = _native.lib()
    E = _native.ERR_INVALID_ARG
    n = C.c_int(-1)
    y, off = (C.c_double * 1)(0.0), (C.c_int64 * 2)(0, 1)
    # a null trainer
    assert L.mrk_train_append_device(None, 0, C.c_void_p(256), 1, 1) == E and b"null trainer" in L.mrk_last_error()
    assert L.mrk_train_seal(None, 0, y, off, 1) == E and b"null trainer" in L.mrk_last_error()
    assert L.mrk_train_seal(None, 1, y, off, 1) == E and b"null trainer" in L.mrk_last_error()
    assert L.mrk_train_bounds(None, 0, None, 0, C.byref(n)) == E and b"null trainer" in L.mrk_last_error()
    assert L.mrk_train_bounds(None, 0, None, 0, None) == E
    assert n.value == -1
    # a bad `which`
    for which in (-1, 2):
        assert L.mrk_train_append_device(None, which, C.c_void_p(256), 1, 1) == E and b"which is neither" in L.mrk_last_error()
        assert L.mrk_train_seal(None, which, y, off, 1) == E and b"which is neither" in L.mrk_last_error()
