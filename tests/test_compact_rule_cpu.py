"""CPU: which pre-pass tables fit the compact 4-byte entry (features.hpp compact_table_ok: at most 2 047 insertions, token ids
below 2^20) and how much dynamic LDS a fused launch asks for at 4 and 8 bytes per entry (launch_shape.hpp fused_lds_bytes), through the
host-only debug export mrk_debug_fused_lds - against the arithmetic written out here."""
import pytest

import metarank_amd as M


def lds(tab_entries, vals_cap, threads, thr_cap, rt_bytes, split, entry_bytes):
    staging = (threads + 63) // 64 * 2 * thr_cap * 8
    rt = rt_bytes if rt_bytes <= (20480 if split else 8192) else 0
    return ((tab_entries * entry_bytes + 7) & ~7) + vals_cap * 8 + 32 * 24 + 96 * 4 + 16 + max(staging, rt)


@pytest.mark.parametrize("insertions,max_token,ok", [(0, 0, True), (1, 1, True), (2047, (1 << 20) - 1, True), (2048, 1, False), (2047, 1 << 20, False),
                                                     (500, 10_000, True), (1 << 40, 5, False), (5, (1 << 32) - 1, False)])
def test_compact_rule(insertions, max_token, ok):
    assert M.debug_fused_lds(insertions, max_token)[0] is ok


@pytest.mark.parametrize("entries", [1, 2, 8, 1374, 1375, 2730, 1 << 20])
@pytest.mark.parametrize("shape", [(1, 64, 0, 0, False), (32, 128, 256, 6040, False), (32, 128, 256, 6040, True), (64, 512, 64, 8200, False), (64, 512, 64, 8200, True),
                                   (4096, 256, 0, 30000, True)])
def test_fused_lds_bytes(entries, shape):
    vals, threads, thr_cap, rt, split = shape
    for eb in (4, 8):
        got = M.debug_fused_lds(0, 0, entries, vals, threads, thr_cap, rt, split, eb)[1]
        assert got == lds(entries, vals, threads, thr_cap, rt, split, eb), (entries, shape, eb)
    wide, compact = (M.debug_fused_lds(0, 0, entries, vals, threads, thr_cap, rt, split, eb)[1] for eb in (8, 4))
    assert wide - compact == entries * 8 - ((entries * 4 + 7) & ~7) and compact % 8 == 0
