"""tests/sort_multi_cases.py — the numpy restatement tests/test_gpu_sort_multi.py compares dfdb_sort_indices_n with — pinned on answers written out by hand
from Julia's sort(df, [:a, :b]; rev = [...]), on an independent statement (Python's sorted over tuple keys) and on np.lexsort; and what of the feature can be
checked without a device: the way of the entry point through the library, the header and the two bindings."""
import os
import re

import numpy as np
import pytest

import order_stat_cases as K
import sort_cases as S
import sort_multi_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def test_two_keys_in_the_four_directions():
    # a = [2, 1, 2, 1, 2, 1], b = [5, 7, 3, 7, 5, 1]
    a = np.array([2, 1, 2, 1, 2, 1], np.int64)
    b = np.array([5, 7, 3, 7, 5, 1], np.int64)
    ref = lambda ra, rb, **kw: M.sortperm_multi_ref([a, b], [None, None], None, [ra, rb], **kw).tolist()
    # sortperm(collect(zip(a, b))): (1,1) (1,7) (1,7) (2,3) (2,5) (2,5); the equal tuples keep their row order
    assert ref(False, False) == [6, 2, 4, 3, 1, 5]
    # rev = [false, true]: a ascending, b descending within it; rows 2, 4 and 1, 5 still ascend
    assert ref(False, True) == [2, 4, 6, 1, 5, 3]
    assert ref(True, False) == [3, 1, 5, 6, 2, 4]
    assert ref(True, True) == [1, 5, 3, 2, 4, 6]
    assert ref(False, True, limit=4) == [2, 4, 6, 1] and ref(False, True, limit=0) == [] and ref(False, True, limit=11) == ref(False, True)
    # under a selection (rows 2..6 of the table): table row numbers come back
    assert M.sortperm_multi_ref([a, b], [None, None], np.arange(1, 6), [False, False]).tolist() == [6, 2, 4, 3, 5]
    # one key is sort_cases' answer; the same column twice orders like the column once
    assert M.sortperm_multi_ref([b], [None], None, [True]).tolist() == S.sortperm_ref(b, rev=True).tolist()
    assert M.sortperm_multi_ref([b, b], [None, None], None, [False, True]).tolist() == S.sortperm_ref(b).tolist()


def test_three_keys_with_mixed_rev():
    a = np.array([1, 1, 1, 1, 0, 0, 1, 1], np.int8)
    b = np.array([2.5, 2.5, 1.5, 2.5, 9.0, 9.0, 1.5, 2.5], np.float32)
    c = np.array([3, 4, 1, 4, 8, 7, 2, 3], np.uint16)
    # a descending, b ascending, c descending: a = 1 first; there b = 1.5 (c: 2, 1 -> rows 7, 3), then b = 2.5 (c: 4, 4, 3, 3 -> rows 2, 4, 1, 8); then a = 0
    # with b = 9.0 twice (c: 8, 7 -> rows 5, 6)
    assert M.sortperm_multi_ref([a, b, c], [None] * 3, None, [True, False, True]).tolist() == [7, 3, 2, 4, 1, 8, 5, 6]


def test_missing_in_the_major_key_the_minor_key_and_both():
    # a = [1, missing, 1, missing, 0], b = [missing, 2, 5, missing, missing]; the bytes under the flags would sort first or last
    a = np.array([1, -99, 1, 99, 0], np.int64)
    am = np.array([0, 1, 0, 1, 0], bool)
    b = np.array([-7, 2, 5, 77, 77], np.int32)
    bm = np.array([1, 0, 0, 1, 1], bool)
    ref = lambda ra, rb: M.sortperm_multi_ref([a, b], [am, bm], None, [ra, rb]).tolist()
    # ascending: a = 0 (row 5), a = 1 (b = 5: row 3, then b missing: row 1), a missing (b = 2: row 2, then b missing: row 4)
    assert ref(False, False) == [5, 3, 1, 2, 4]
    # b descending: missing in b comes first within equal a
    assert ref(False, True) == [5, 1, 3, 4, 2]
    # a descending: missing in a first
    assert ref(True, False) == [2, 4, 3, 1, 5]
    assert ref(True, True) == [4, 2, 1, 3, 5]
    assert M.info_multi_ref([a, b], [am, bm]) == (5, 3 + 2, 1 + 1, 7 + 3)            # a's live values 1, 1, 0: one byte varies; b's 2, 5: one byte
    assert M.info_multi_ref([a, b], [am, bm], np.array([1, 3])) == (2, 0 + 1, 0, 8 + 4)


def test_signed_zeros_and_nans_tie_on_nothing_and_the_minor_key_breaks_real_ties():
    # isless: -0.0 < 0.0 < NaN, and every NaN is one value
    x = np.array([0.0, -0.0, NAN, 0.0, -0.0, NAN])
    x.view(np.uint64)[5] = np.uint64(0xfff8000000000dea)            # another NaN: the same key
    y = np.array([3, 2, 1, 1, 5, 0], np.int64)
    # x ascending: -0.0 (rows 2, 5), 0.0 (rows 1, 4), NaN (rows 3, 6); y ascending inside: 2 < 5; 1 < 3 -> rows 4, 1; 0 < 1 -> rows 6, 3
    assert M.sortperm_multi_ref([x, y], [None, None]).tolist() == [2, 5, 4, 1, 6, 3]
    assert M.sortperm_multi_ref([x, y], [None, None], None, [True, True]).tolist() == [3, 6, 1, 4, 5, 2]
    f = x.astype(np.float32)
    assert M.sortperm_multi_ref([f, y], [None, None]).tolist() == [2, 5, 4, 1, 6, 3]


def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    nk = int(rng.integers(1, 5))
    cols, missings = [], []
    for _ in range(nk):
        kind = rng.integers(0, 4)
        if kind == 0:
            c = rng.integers(-2, 3, n).astype(np.int8)
        elif kind == 1:
            c = rng.choice(np.array([0.0, -0.0, 1.5, -np.inf, np.inf, NAN]), n)
        elif kind == 2:
            c = rng.integers(0, 3, n).astype(np.uint64) << np.uint64(62)
        else:
            c = rng.random(n) < 0.5
        cols.append(c)
        missings.append(rng.random(n) < 0.3 if rng.random() < 0.5 else None)
    rows = np.flatnonzero(rng.random(n) < 0.8) if rng.random() < 0.5 else None
    revs = [bool(r) for r in rng.random(nk) < 0.5]
    return cols, missings, rows, revs


@pytest.mark.parametrize("seed", range(40))
def test_against_sorted_over_tuple_keys(seed):
    cols, missings, rows, revs = random_case(seed)
    n = len(cols[0])
    sel = range(n) if rows is None else [int(r) for r in rows]

    def key(r):
        parts = []
        for c, m, rev in zip(cols, missings, revs):
            gone = m is not None and bool(m[r])
            img = 0 if gone else int(K.image(np.ascontiguousarray(c)[r:r + 1])[0])
            parts += [(0 if gone else 1) if rev else (1 if gone else 0), -img if rev else img]
        return tuple(parts) + (r,)

    want = [r + 1 for r in sorted(sel, key=key)]
    assert M.sortperm_multi_ref(cols, missings, rows, revs).tolist() == want
    assert M.sortperm_multi_ref(cols, missings, rows, revs, 3).tolist() == want[:3]


@pytest.mark.parametrize("seed", range(10))
def test_against_lexsort_where_nothing_is_missing_or_reversed(seed):
    rng = np.random.default_rng([seed, 77])
    n = 500
    cols = [rng.integers(0, 4, n).astype(np.int64), rng.integers(-3, 3, n).astype(np.int16), rng.standard_normal(n).round(1) + 0.0]       # (+ 0.0: no -0.0, which lexsort ties with 0.0 and isless does not)
    want = np.lexsort(tuple(reversed(cols))) + 1                    # (lexsort's LAST key is the major one; it is stable)
    assert np.array_equal(M.sortperm_multi_ref(cols, [None] * 3), want)


def test_pairs_and_passes_sum_over_the_keys():
    n = 1025
    eq, lo, b = K.shape_column("equal", n), K.shape_column("low_byte", n), K.shape_column("bool", n)
    assert M.info_multi_ref([eq, lo, b], [None] * 3) == (n, 3 * n, 0 + 1 + 1, 8 + 7 + 0)
    x, m = K.nullable_column(n, all_missing=True)
    assert M.info_multi_ref([x, lo], [m, None]) == (n, n, 1, 8 + 7)
    assert M.info_multi_ref([lo, lo], [None, None], np.zeros(0, np.int64)) == (0, 0, 0, 16)


def test_the_entry_point_goes_through_every_layer():
    from dfdb import _native as N
    symbol = "dfdb_sort_indices_n"
    assert symbol in N.SYMBOLS and len(getattr(N.load(), symbol).argtypes) == 10                             # exported and bound
    header = open(os.path.join(ROOT, "include", "dfdb.h")).read()
    assert re.search(r"^int32_t %s\(" % symbol, header, re.M)
    shim = open(os.path.join(ROOT, "dataframedbs.jl_amd", "julia", "DataFrameDBsAMD.jl")).read()
    assert "ccall((:%s, LIB)" % symbol in shim
    assert "DFDB_SORT_MAX_KEYS = 8" in header and N.SORT_MAX_KEYS == 8
    import dfdb
    assert dfdb.SORT_MAX_KEYS == 8 and callable(dfdb.sortperm_by) and hasattr(dfdb.api._Query, "sort_indices_n")
