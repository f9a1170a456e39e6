"""CPU: the per-column distinct-token tracker of the feature store (csrc/store.hpp Column::distinct) - the bound the pre-pass
hash tables are sized by - against sets kept by the test (tests/native/distinct_test.cpp): puts through every entry point
that can write a string cell (C-string and KeyRef forms, the binary loader), overwrites, erases, clones.  store.cpp,
features.cpp and codec.cpp are compiled INTO the test binary with AddressSanitizer + UBSan; the rest comes from
libmrk_hip.so.  No device."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_distinct_count_bounds_every_column_vocabulary(tmp_path):
    from metarank_amd import _native

    _native.build()
    exe = str(tmp_path / "distinct_test")
    lib_dir = os.path.dirname(_native.LIB_PATH)
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", os.path.join(REPO, "tests", "native", "distinct_test.cpp"), os.path.join(csrc, "store.cpp"),
                           os.path.join(csrc, "features.cpp"), os.path.join(csrc, "codec.cpp"), "-I" + csrc, "-I" + os.path.join(REPO, "include"),
                           "-L" + lib_dir, "-lmrk_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert " 0 bad" in out.stdout and "genre 3 " in out.stdout
