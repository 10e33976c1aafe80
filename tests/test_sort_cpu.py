"""tests/sort_cases.py — the numpy restatement tests/test_gpu_sort.py compares dfdb_sort_indices with — pinned on answers written out by hand from Julia's
sortperm / partialsortperm, and what of the feature can be checked without a device: the chunk geometry self-test and the way of both entry points
through the library, the header and the two bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import order_stat_cases as K
import sort_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_floats_in_both_directions():
    x = np.array([2.0, -0.0, NAN, 0.0, -INF, 2.0])
    # sortperm([2.0, -0.0, NaN, 0.0, -Inf, 2.0]): -Inf < -0.0 < 0.0 < 2.0 (rows 1, 6) < NaN
    assert S.sortperm_ref(x).tolist() == [5, 2, 4, 1, 6, 3]
    # sortperm(...; rev = true): NaN first; the two 2.0 keep their row order
    assert S.sortperm_ref(x, rev=True).tolist() == [3, 1, 6, 4, 2, 5]
    f = x.astype(np.float32)
    assert S.sortperm_ref(f).tolist() == [5, 2, 4, 1, 6, 3] and S.sortperm_ref(f, rev=True).tolist() == [3, 1, 6, 4, 2, 5]


def test_missing_last_ascending_and_first_under_rev():
    # x = Union{Int,Missing}[3, missing, 1, missing, 2, 1]; the bytes under the missing flags would sort first and last
    x = np.array([3, -99, 1, 99, 2, 1], np.int64)
    m = np.array([0, 1, 0, 1, 0, 0], bool)
    assert S.sortperm_ref(x, m).tolist() == [3, 6, 5, 1, 2, 4]
    assert S.sortperm_ref(x, m, rev=True).tolist() == [2, 4, 1, 5, 3, 6]
    # under a selection (rows 2..6 of the table): table row numbers come back
    rows = np.arange(1, 6)
    assert S.sortperm_ref(x, m, rows).tolist() == [3, 6, 5, 2, 4]
    assert S.sortperm_ref(x, m, rows, rev=True).tolist() == [2, 4, 5, 3, 6]


def test_limit_is_a_prefix_and_the_cut_keeps_every_tie():
    x = np.array([5, 1, 3, 1, 5, 2, 5], np.int64)
    full = S.sortperm_ref(x).tolist()
    assert full == [2, 4, 6, 3, 1, 5, 7]
    assert S.sortperm_ref(x, limit=0).tolist() == [] and S.sortperm_ref(x, limit=1).tolist() == [2]          # partialsortperm(x, 1:1)
    assert S.sortperm_ref(x, limit=len(x) + 5).tolist() == full
    assert S.sortperm_ref(x, rev=True, limit=2).tolist() == [1, 5]                                           # the smallest rows among the tied 5s
    assert S.candidates_ref(x, limit=0) == 0 and S.candidates_ref(x, limit=1) == 2                           # both 1s
    assert S.candidates_ref(x, limit=3) == 3 and S.candidates_ref(x, limit=7) == 7 and S.candidates_ref(x, limit=12) == 7
    assert S.candidates_ref(x, rev=True, limit=1) == 3 and S.candidates_ref(x, limit=None) == 7              # the three 5s
    m = np.array([0, 0, 0, 0, 0, 0, 1], bool)                                                                # the last 5 is missing
    assert S.sortperm_ref(x, m, rev=True, limit=2).tolist() == [7, 1]
    assert S.candidates_ref(x, m, rev=True, limit=1) == 0 and S.candidates_ref(x, m, rev=True, limit=2) == 2
    assert S.candidates_ref(x, m, limit=6) == 6 and S.candidates_ref(x, m, limit=7) == 6


def test_pass_counts():
    n = 1025
    assert S.passes_ref(K.shape_column("equal", n)) == (0, 8)
    assert S.passes_ref(K.shape_column("low_byte", n)) == (1, 7) and S.passes_ref(K.shape_column("high_byte", n)) == (1, 7)
    below_1e6 = np.random.default_rng(1).integers(0, 1_000_000, 70_001).astype(np.int64)
    assert S.passes_ref(below_1e6) == (3, 5)
    assert S.passes_ref(K.shape_column("bool", n)) == (1, 0) and S.passes_ref(K.shape_column("int16", n)) == (2, 0)
    x, m = K.nullable_column(n, all_missing=True)
    assert S.passes_ref(x, m) == (0, 8)                                                                      # no pair, no pass: none for the missing flag either
    assert S.passes_ref(np.array([5, 1, 3, 1, 5, 2, 5], np.int64), limit=1) == (0, 8)                        # the candidates are the two 1s


@pytest.mark.parametrize("shape", K.SHAPES)
def test_the_narrow_key_orders_like_the_image(shape):
    x = K.shape_column(shape, 1025)
    assert np.array_equal(np.argsort(S.narrow_key(x), kind="stable"), np.argsort(K.image(x), kind="stable"))
    assert int(S.narrow_key(x).max()) >> (8 * S.key_bytes(x.dtype) - 1) <= 1


def test_sort_geometry_answers_without_a_device():
    from dfdb import _native as N
    out = (C.c_int64 * 2)()
    assert N.load().dfdb_selftest(b"sort_geometry", 0, out, 2) == 0
    chunk, threads = out[0], out[1]
    assert threads > 0 and threads % 64 == 0 and chunk > 0 and chunk % threads == 0
    assert N.load().dfdb_selftest(b"sort_geometry", 0, out, 1) == N.ERR_ARGUMENT


@pytest.mark.parametrize("symbol", ["dfdb_sort_indices", "dfdb_gather_rows"])
def test_both_entry_points_go_through_every_layer(symbol):
    from dfdb import _native as N
    assert symbol in N.SYMBOLS and getattr(N.load(), symbol).argtypes is not None                           # exported and bound
    header = open(os.path.join(ROOT, "include", "dfdb.h")).read()
    assert re.search(r"^int32_t %s\(" % symbol, header, re.M)
    shim = open(os.path.join(ROOT, "dataframedbs.jl_amd", "julia", "DataFrameDBsAMD.jl")).read()
    assert "ccall((:%s, LIB)" % symbol in shim
    assert "DFDB_SORT_REV = 1" in header and N.SORT_REV == 1
