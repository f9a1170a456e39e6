"""Which kernel a dense product of a split-bf16 encoder handle runs (split_launch_plan, metarank_amd/csrc/launch_shape.hpp): host
arithmetic through mrk_debug_split_plan, no device.  MRK_ENCODER_SPLIT_SKINNY at its shipped default (1) unless a row sets it."""
import ctypes as C
import os

import pytest

from metarank_amd import _native

SKINNY, TILE_32x64, TILE_64, TILE_128 = range(4)   # SplitKernel


@pytest.mark.parametrize("M,N,K,switch,want,why", [
    *[(m, 64, 64, None, (SKINNY, 2, 256), "the smallest model: one k step per wavefront") for m in (1, 9, 32)],
    *[(m, 384, 1536, None, (SKINNY, 12, 256), "MiniLM's FFN 2: N / 32 workgroups of four wavefronts") for m in (1, 9, 32)],
    (32, 384, 384, "0", (TILE_32x64, 6, 128), "MRK_ENCODER_SPLIT_SKINNY=0: the 32 x 64 tile, N / 64 workgroups of two wavefronts"),
    (32, 64, 96, None, (TILE_32x64, 1, 128), "K % 64 != 0: the k steps do not divide over four wavefronts"),
    (33, 384, 384, None, (TILE_64, 8 * 6, 256), "one row more: 64 x 64 tiles on the XCD fold's grid"),
    (5670, 384, 384, None, (TILE_64, 8 * 12 * 6, 256), "the 128 x 128 rule: 45 x 3 = 135 of them do not cover the chip, 64 x 64 tiles stay"),
    (5670, 768, 768, None, (TILE_128, 8 * 6 * 6, 256), "... 45 x 6 = 270 >= 256 do"),
])
def test_split_launch_plan(M, N, K, switch, want, why):
    L = _native.lib()
    L.mrk_debug_split_plan.restype = C.c_int
    L.mrk_debug_split_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * 3)()
    if switch is not None:
        os.environ["MRK_ENCODER_SPLIT_SKINNY"] = switch
        _native.reload_switches()
    try:
        assert L.mrk_debug_split_plan(M, N, K, out) == 0
    finally:
        if switch is not None:
            del os.environ["MRK_ENCODER_SPLIT_SKINNY"]
            _native.reload_switches()
    assert tuple(out) == want, why
