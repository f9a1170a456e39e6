"""CPU: the bit-vector scorer's byte-mode image (forest.cpp pack_forest_qs, PackedForestQS::bnodes) and tree step, emulated
bit for bit on the host (tests/native/qs_byte_test.cpp: v_pk_min_u16 clamp, v_pk_sub_i16 wraparound, the two v_and_or_b32
ladders, the v_perm_b32 merge, categorical nodes on unclamped cells) - every exit leaf against the 16-bit QuickScorer rule
and a plain tree walk, for every cell in [0, 255] and 0x7FFF on every node's view: random trees, left / right combs,
trees of fewer than 16 leaves, 255 thresholds on a column (k = 254), per-node missing rules, categorical nodes; a column of
256 thresholds is refused byte mode.  ASan + UBSan."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_byte_mode_step_matches_16_bit_rule(tmp_path):
    exe = str(tmp_path / "qs_byte_test")
    csrc = os.path.join(REPO, "metarank_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(REPO, "tests", "native", "qs_byte_test.cpp"), os.path.join(csrc, "forest.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ALL OK" in out.stdout
    assert "256 thresholds on a column: byte mode refused" in out.stdout
    assert "left and right combs:" in out.stdout and "max 7" in out.stdout.split("left and right combs:")[1].split("\n")[0]
