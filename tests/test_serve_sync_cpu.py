"""CPU: the serving queue's synchronisation pieces (csrc/serve_sync.hpp: reader gate, slot pool, overflow window) -
tests/native/serve_sync_test.cpp as a stand-alone program, once under ASan + UBSan and once under TSan.  The driver includes
serve_sync.hpp alone and is compiled by g++ without a HIP include path: the header is free of HIP."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_serve_sync_native_driver(tmp_path, sanitizer):
    exe = str(tmp_path / "serve_sync_test")
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(REPO, "tests", "native", "serve_sync_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ALL OK" in out.stdout
