"""tests/sort_str_cases.py — the restatement tests/test_order_by_string_gpu.py compares dfdb_sort_indices_any with — pinned on answers written out by hand from
Julia's rules for isless on Strings (bytes unsigned, the shorter of two that tie is smaller, a NUL is a byte), on an independent statement (Python's sorted
over bytes / tuple keys with a stable descending rule); and what of the feature can be checked without a device: the entry point's way through the library,
the header and the two bindings."""
import os
import re

import numpy as np
import pytest

import order_stat_cases as K
import sort_str_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def perm(values, rev=False, rows=None, limit=None):
    return T.sortperm_any_ref([list(values)], [None], rows, [rev], limit).tolist()


def in_order(strings):
    """`strings` written in ascending order, handed over shuffled: the restatement must bring them back (and reversed under rev)"""
    rng = np.random.default_rng(len(strings))
    p = rng.permutation(len(strings))
    shuffled = [strings[i] for i in p]
    back = [shuffled[r - 1] for r in perm(shuffled)]
    down = [shuffled[r - 1] for r in perm(shuffled, rev=True)]
    return back == list(strings) and down == list(reversed(strings))


def test_shorter_is_smaller_and_a_nul_is_a_byte():
    assert in_order([b"", b"a", b"a\0", b"a\0\0", b"ab", b"b"])
    assert in_order([b"abcdefgh", b"abcdefgh\0", b"abcdefghi"])                  # the tie of a whole chunk is broken by the next chunk, then by the length
    assert in_order([b"abcdefg", b"abcdefg\0", b"abcdefg\0\0", b"abcdefg\0\0\0", b"abcdefg\0\1"])


def test_bytes_compare_unsigned():
    assert in_order(["z".encode(), "é".encode()])                               # 0x7a < 0xc3 0xa9
    assert in_order([b"\x7f", b"\x80", b"\xff", b"\xff\x00"])
    assert in_order(["a".encode(), "ab".encode(), "aé".encode(), "b".encode(), "é".encode(), "日本".encode(), "日本語".encode()])


def test_a_difference_in_byte_9_and_in_byte_17():
    assert in_order([b"12345678A", b"12345678B", b"12345678B0", b"12345679"])
    assert in_order([b"1234567812345678A", b"1234567812345678B", b"1234567812345679", b"123456782"])
    keys, miss = T.sub_keys([b"1234567812345678A", b"1", None])
    assert len(keys) == 4 and keys[3].tolist() == [17, 1, 0] and miss.tolist() == [False, False, True]
    assert keys[0][1] == 0x31 << 56 and keys[1][1] == 0 and keys[2][0] == 0x41 << 56


def test_missing_sorts_last_and_first_under_rev_and_ties_keep_row_order():
    v = [b"b", None, b"a", b"b", None, b"a", b""]
    assert perm(v) == [7, 3, 6, 1, 4, 2, 5]
    assert perm(v, rev=True) == [2, 5, 1, 4, 3, 6, 7]                            # the ties 1, 4 and 3, 6 and the missing rows 2, 5 still ascend
    assert perm(v, limit=3) == [7, 3, 6] and perm(v, limit=0) == [] and perm(v, limit=99) == perm(v)
    assert perm(v, rows=np.array([0, 1, 3, 5])) == [6, 1, 4, 2]                  # under a selection: table rows come back
    assert perm([None, None]) == [1, 2] and perm([None, None], rev=True) == [1, 2]


def test_string_keys_beside_numeric_ones():
    s = [b"x", b"y", b"x", None, b"y", b"x"]
    a = np.array([3, 1, 2, 9, 1, 2], np.int64)
    ref = lambda cols, revs: T.sortperm_any_ref(cols, [None] * len(cols), None, revs).tolist()
    assert ref([s, a], [False, False]) == [3, 6, 1, 2, 5, 4]                     # x: a = 2 (rows 3, 6), 3 (row 1); y: a = 1 (rows 2, 5); missing
    assert ref([s, a], [True, False]) == [4, 2, 5, 3, 6, 1]
    assert ref([a, s], [False, True]) == [2, 5, 3, 6, 1, 4]                      # a = 1: y, y; a = 2: x, x; 3; 9
    assert ref([s, s], [False, True]) == ref([s], [False])                       # the major copy decides


def stable_sorted(sel, cols, revs):
    """the independent statement: one stable pass of Python's sorted per key, the most minor first; descending = ascending on the reversed list, reversed
    (stable for ties in ascending row order both ways); missing last, first under rev"""
    order = list(sel)
    for c, rev in reversed(list(zip(cols, revs))):
        val = (lambda r: c[r]) if T.is_string_key(c) else (lambda r: int(K.image(np.ascontiguousarray(c)[r:r + 1])[0]))
        live = [r for r in order if not (T.is_string_key(c) and c[r] is None)]
        miss = [r for r in order if T.is_string_key(c) and c[r] is None]
        if rev:
            live = list(reversed(sorted(reversed(live), key=val)))
        else:
            live = sorted(live, key=val)
        order = miss + live if rev else live + miss
    return [r + 1 for r in order]


ALPHABET = [b"", b"a", b"ab", b"a\0", b"abcdefgh", b"abcdefgh\0", b"abcdefghi", b"abcdefgha", "é".encode(), b"z", b"0123456789abcdefX", b"0123456789abcdefY", None]


@pytest.mark.parametrize("seed", range(40))
def test_against_sorted_over_bytes_and_tuple_keys(seed):
    rng = np.random.default_rng([seed, 5])
    n = int(rng.integers(1, 60))
    nk = int(rng.integers(1, 4))
    cols = []
    for j in range(nk):
        if j == 0 or rng.random() < 0.6:
            cols.append([ALPHABET[i] for i in rng.integers(0, len(ALPHABET), n)])
        else:
            cols.append(rng.integers(-2, 3, n).astype(np.int8))
    revs = [bool(r) for r in rng.random(nk) < 0.5]
    rows = np.flatnonzero(rng.random(n) < 0.8) if rng.random() < 0.5 else None
    want = stable_sorted(range(n) if rows is None else [int(r) for r in rows], cols, revs)
    assert T.sortperm_any_ref(cols, [None] * nk, rows, revs).tolist() == want
    assert T.sortperm_any_ref(cols, [None] * nk, rows, revs, 3).tolist() == want[:3]


def test_info_counts_every_sub_key():
    v = [b"abcdefghi", b"abcdefghj", None, b"abc"]                              # L = 9: two chunks and the length
    # pairs: 3 live rows x 3 sub-keys; length 9, 9, 3: one byte varies; chunk 1 'i', 'j', nothing: its top byte; chunk 0 "abcdefgh" x 2, "abc": bytes 4..0 vary
    assert T.info_any_ref([v], [None]) == (4, 9, 1 + 1 + 5, 7 + 7 + 3)
    assert T.info_any_ref([v], [None], np.array([2, 3])) == (2, 2, 0, 16)       # the selection decides m: "abc" alone, one chunk
    assert T.info_any_ref([[b"", b""]], [None]) == (2, 2, 0, 8)                 # all empty: m = 0, the length alone, every pass skipped
    assert T.info_any_ref([[b"q"] * 5], [None]) == (5, 10, 0, 16)               # all equal
    assert T.info_any_ref([[None, None]], [None]) == (2, 0, 0, 8)
    a = np.array([1, 2, 1, 2], np.int64)
    assert T.info_any_ref([a, v], [None, None]) == (4, 4 + 9, 1 + 7, 7 + 17)
    assert T.info_any_ref([a], [None], None, [False], 1) == (4, 2, 0, 8)        # numeric keys only: dfdb_sort_indices_n's answer, the top-k cut included


def test_the_entry_point_goes_through_every_layer():
    import dfdb
    from dfdb import _native as N
    assert dfdb.SORT_MAX_STRING_BYTES == 256 == T.MAX_STRING_BYTES
    assert hasattr(dfdb.api._Query, "sort_indices_any")
    assert "dfdb_sort_indices_any" in dfdb.SYMBOLS
    header = open(os.path.join(ROOT, "include", "dfdb.h")).read()
    assert re.search(r"^int32_t dfdb_sort_indices_any\(", header, re.M) and "DFDB_SORT_MAX_STRING_BYTES = 256" in header
    assert len(getattr(N.load(), "dfdb_sort_indices_any").argtypes) == 10      # exported and bound
    shim = open(os.path.join(ROOT, "dataframedbs.jl_amd", "julia", "DataFrameDBsAMD.jl")).read()
    assert "ccall((:dfdb_sort_indices_any, LIB)" in shim
