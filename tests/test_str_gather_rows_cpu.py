"""What the String gather at given rows (dfdb_gather_rows_any) rests on and needs no GPU: the definition tests/str_gather_rows_cases.py states, on hand-written
answers; the two entry points in the Python symbol table and in the header; the rule between the gather's two forms at its boundary (dfdb_selftest
"str_gather_form": direct when n * 512 <= nrows)."""
import ctypes as C
import os
import re

import numpy as np

import str_gather_rows_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_take_ref_on_hand_written_answers():
    values = ["ab", None, "", "héé", "z"]
    sizes, data = G.take_ref(values, [4, 2, 3, 1, 1, 5])                  # a multi-byte string, a missing row, an empty string, a repeat
    assert sizes.dtype == np.int32 and sizes.tolist() == [5, -1, 0, 2, 2, 1]
    assert data.dtype == np.uint8 and data.tobytes() == "héé".encode() + b"ab" + b"ab" + b"z"
    sizes, data = G.take_ref(values, [])
    assert sizes.tolist() == [] and len(data) == 0
    sizes, data = G.take_ref(values, [2, 2])
    assert sizes.tolist() == [-1, -1] and len(data) == 0
    sizes, data = G.take_ref(values, [5, 4, 3, 2, 1])
    assert sizes.tolist() == [1, 5, 0, -1, 2] and data.tobytes() == b"z" + "héé".encode() + b"ab"


def test_case_columns_cover_every_length_and_both_kinds_of_missing():
    cols = G.columns(2049)
    assert {len(s.encode()) for s in cols["plain"]} == set(G.LENGTHS)
    assert any(len(s) != len(s.encode()) for s in cols["plain"])          # multi-byte UTF-8 is there
    assert [i for i, s in enumerate(cols["fifth"]) if s is None] == list(range(4, 2049, 5))
    assert [i for i, s in enumerate(cols["tile"]) if s is None] == list(range(1024, 2048))
    for nrows in G.COLUMN_ROWS:
        for name, rows in G.row_lists(nrows).items():
            assert rows.dtype == np.int64 and (len(rows) == 0 or (rows.min() >= 1 and rows.max() <= nrows)), (nrows, name)
    assert len(G.row_lists(70_001)["repeat1500"]) == 1500 and len(set(G.row_lists(70_001)["repeat1500"].tolist())) == 1


def test_both_entry_points_are_bound_and_declared():
    import dfdb
    header = open(os.path.join(ROOT, "include", "dfdb.h")).read()
    for name in ("dfdb_gather_rows_string_bytes", "dfdb_gather_rows_any"):
        assert name in dfdb.SYMBOLS
        assert re.search(r"^int32_t %s\(dfdb_query\* q, " % name, header, re.M), name
    assert callable(dfdb.take)


def gather_form(n, nrows, forced=0):
    from dfdb import _native as N
    out = (C.c_int64 * 3)(n, nrows, forced)
    N.check(N.load().dfdb_selftest(b"str_gather_form", 0, out, 3))
    return int(out[0])


def test_form_rule_at_its_boundary():
    OFFSETS, DIRECT = 1, 2
    for nrows in (512, 70_001, 500_000_000):
        edge = nrows // 512                                               # the largest n with n * 512 <= nrows
        assert edge * 512 <= nrows < (edge + 1) * 512
        assert gather_form(edge, nrows) == DIRECT and gather_form(edge + 1, nrows) == OFFSETS, nrows
    assert gather_form(1, 511) == OFFSETS and gather_form(1, 512) == DIRECT
    assert gather_form(10, 500_000_000) == DIRECT                         # a top-10 of a long column builds no column-wide array
    assert gather_form(100_000_000, 500_000_000) == OFFSETS
    for n, nrows in ((1, 1), (10, 500_000_000), (70_001, 70_001)):        # the context option "str_gather_form" overrides the rule both ways
        assert gather_form(n, nrows, OFFSETS) == OFFSETS and gather_form(n, nrows, DIRECT) == DIRECT
        assert gather_form(n, nrows, 3) == gather_form(n, nrows)
