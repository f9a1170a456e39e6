"""CPU: the lane rule of the wavefront-per-request ordering (csrc/sort_device.hpp sort_wave_step, walked as rank.hip sort_wave_kernel
walks it) compiled for the HOST (tests/native/sort_wave_test.cpp): 64 simulated lanes against std::stable_sort on (sort_key, index) for
n = 0, 1, 2, 63, 64, 65, 100, 127, 128 and keys all equal, strictly descending, strictly ascending, NaNs of both signs, +-0, +-inf and
runs of ties that straddle lanes 63 / 64.  A stand-alone program under ASan + UBSan."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lane_counts_are_the_stable_order(tmp_path):
    exe = str(tmp_path / "sort_wave_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I" + os.path.join(REPO, "metarank_amd", "csrc"), os.path.join(REPO, "tests", "native", "sort_wave_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "sort wave rule:" in out.stdout and " 0 bad" in out.stdout
