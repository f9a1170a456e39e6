"""LDS of the one-request kernel that walks deep forests (metarank_amd/csrc/launch_shape.hpp rank_one_walk_lds_bytes): host
arithmetic, no device - the same route as tests/test_launch_shapes_cpu.py."""
import ctypes as C

import pytest

from metarank_amd import _native

CAP = 96 * 1024
CHUNK = 24 * 1024          # score.hip's chunk budget
ASSEMBLY = 20 * 1024       # a request's hash tables and scratch: what the pre-pass and assembly phase keep in LDS


@pytest.fixture(scope="module")
def lds():
    L = _native.lib()
    L.mrk_debug_walk_lds.restype = C.c_int64
    L.mrk_debug_walk_lds.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int64, C.POINTER(C.c_int)]

    def f(cols, f64, chunk_bytes=CHUNK, chunk_trees=19, assembly=ASSEMBLY):
        lt = C.c_int(0)
        n = L.mrk_debug_walk_lds(cols, 1 if f64 else 0, chunk_bytes, chunk_trees, assembly, C.byref(lt))
        return n, lt.value
    return f


def expected(cols, f64, chunk_bytes, chunk_trees, assembly):
    esz = 8 if f64 else 4
    up = lambda x: (x + 15) // 16 * 16
    leaf_trees = max(1, min(chunk_trees, 32))
    scoring = up(chunk_bytes) + up(chunk_trees * 12) + max(leaf_trees * 128 * esz, 1024)
    return cols * 128 * esz + 16 + max(assembly, scoring)


@pytest.mark.parametrize("cols,f64,chunk_bytes,chunk_trees,assembly", [
    (24, False, CHUNK, 19, ASSEMBLY), (24, True, CHUNK, 65, ASSEMBLY), (64, True, CHUNK, 4, ASSEMBLY), (1, False, 16, 1, 0),
    (24, True, 5104, 1, 60 * 1024), (0, True, 0, 0, 0)])
def test_the_four_regions_add_up(lds, cols, f64, chunk_bytes, chunk_trees, assembly):
    n, lt = lds(cols, f64, chunk_bytes, chunk_trees, assembly)
    assert n == expected(cols, f64, chunk_bytes, chunk_trees, assembly)
    assert lt == max(1, min(chunk_trees, 32))


def test_monotone_in_columns_chunk_bytes_and_element_width(lds):
    for f64 in (False, True):
        prev = 0
        for cols in range(0, 130):
            n, _ = lds(cols, f64)
            assert n > prev
            prev = n
        prev = 0
        for chunk in range(0, 64 * 1024, 1024):
            n, _ = lds(24, f64, chunk_bytes=chunk, assembly=0)
            assert n >= prev and (chunk == 0 or n > prev)
            prev = n
    for cols in (1, 24, 64):
        for trees in (1, 4, 19, 65):
            assert lds(cols, True, chunk_trees=trees)[0] > lds(cols, False, chunk_trees=trees)[0]


def test_the_scoring_regions_overlay_the_assembly_regions(lds):
    small, _ = lds(24, True, assembly=1024)
    assert lds(24, True, assembly=2048)[0] == small          # below the scoring regions: free
    assert lds(24, True, assembly=90 * 1024)[0] == 24 * 128 * 8 + 16 + 90 * 1024


@pytest.mark.parametrize("cols,f64,fits", [(24, False, True), (24, True, True), (64, True, False)])
def test_the_96_kb_boundary(lds, cols, f64, fits):
    """A 24 KB chunk of depth-6 XGBoost trees (19) or 16-leaf LightGBM trees (65): 24 columns fit in either precision, the 64 f64
    columns of the c3 program (64 KB of matrix) do not - such a model keeps its three launches."""
    for trees in (19, 65):
        n, _ = lds(cols, f64, chunk_trees=trees)
        assert (n <= CAP) == fits, (cols, f64, trees, n)
    # the boundary itself: the largest assembly size that still fits, and one 16-byte step beyond
    if fits:
        n0, _ = lds(cols, f64, assembly=0)
        room = CAP - (cols * 128 * (8 if f64 else 4) + 16)
        assert n0 <= CAP and lds(cols, f64, assembly=room)[0] == CAP and lds(cols, f64, assembly=room + 16)[0] > CAP
