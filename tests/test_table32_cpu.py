"""CPU: the compact 4-byte entries of the pre-pass hash tables (csrc/table32_device.hpp - the tables mrk_jit_rank_cells keeps in
LDS) compiled for the HOST with the one-lane stand-in for the wavefront primitives (tests/native/table32_test.cpp): against a
std::map and, entry by entry, against the 8-byte tables of table_device.hpp; six host threads inserting into one table; a key
counted exactly 2 047 times; token ids 1 and 2^20 - 1; tables at and past their load bound (walked-past marks); tables that start
8 but not 16 bytes into an aligned block, with guard words around them.  A stand-alone program under ASan + UBSan."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compact_tables_agree_with_a_map_and_with_the_wide_tables(tmp_path):
    exe = str(tmp_path / "table32_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(REPO, "metarank_amd", "csrc"), os.path.join(REPO, "tests", "native", "table32_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "compact tables, PROBE_W 4:" in out.stdout and " 0 bad" in out.stdout
