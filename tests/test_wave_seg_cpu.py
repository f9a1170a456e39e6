"""CPU: the lane mapping of the all-lanes pre-pass (csrc/wave_device.hpp: wave_nth_set, wave_seg_source, iw_task_rounds, iw_task_of)
compiled for the HOST (tests/native/wave_seg_test.cpp): the segmented median (wave_seg_median_of) bit for bit against wave_median_of per
segment (n = 0, 1, 2, 19, 20, odd, even; NaNs, all NaN, +-0, duplicates), the segmented selection against a per-segment serial prefix count (segment
widths 1, 3, 20, 21, 32, 64; flags all set, none, alternating, random; segments that fill the wavefront and that do not), and the
dealing of the interacted_with tasks - every (item, field) exactly once for lists of 0 .. 100 items and 1 .. 4 fields, by stride and
from one counter in any interleaving of two claimers.  A stand-alone program under ASan + UBSan."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segments_and_tasks_cover_exactly_once(tmp_path):
    exe = str(tmp_path / "wave_seg_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(REPO, "metarank_amd", "csrc"), os.path.join(REPO, "tests", "native", "wave_seg_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "wave segments and tasks:" in out.stdout and " 0 bad" in out.stdout
