"""CPU: the error boundary of the C ABI (csrc/status.hpp) - tests/native/status_test.cpp under ASan + UBSan.  The driver includes
status.hpp and forest.hpp alone and is compiled by g++ without a HIP include path: the header the *_host.cpp halves share is
free of HIP."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_status_native_driver(tmp_path):
    exe = str(tmp_path / "status_test")
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(REPO, "tests", "native", "status_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ALL OK" in out.stdout
