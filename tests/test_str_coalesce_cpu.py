"""The yardstick of tests/test_gpu_str_coalesce.py pinned without a GPU: the restatement of coalesce over Strings (str_coalesce_cases.coalesce_ref) against
a literal known-answer table, its flat form, the case table's own claims, and the IR bytes the front end produces for coalesce(col, "x") and string(col)."""
import struct

import numpy as np

import str_coalesce_cases as K
from str_coalesce_cases import coalesce_ref, flat, unflat

NON_ASCII = "é→".encode() + b"\xff"


def test_known_answers():
    a = [b"x", None, b"", None, b"a\0b", None]
    b = [b"1", b"2", b"3", None, None, b""]
    assert coalesce_ref(a, b) == [b"x", b"2", b"", None, b"a\0b", b""]              # a missing a; missing in both stays missing; "" is a value, not missing
    assert coalesce_ref(a, b"") == [b"x", b"", b"", b"", b"a\0b", b""]              # the tutorial's string_convert: the constant ""
    assert coalesce_ref(a, b"missing") == [b"x", b"missing", b"", b"missing", b"a\0b", b"missing"]
    assert coalesce_ref(a, NON_ASCII) == [b"x", NON_ASCII, b"", NON_ASCII, b"a\0b", NON_ASCII]
    assert coalesce_ref([b"p", b"", b"q"], [None, None, b"z"]) == [b"p", b"", b"q"]  # a non-nullable a gives a back
    assert coalesce_ref([None] * 3, b"") == [b""] * 3 and coalesce_ref([], b"d") == []


def test_flat_form_known_answers():
    vals = [b"ab", None, b"", NON_ASCII, None]
    sizes, data, total = flat(vals)
    assert sizes.dtype == np.int32 and sizes.tolist() == [2, -1, 0, len(NON_ASCII), -1]
    assert data.tobytes() == b"ab" + NON_ASCII and total == 2 + len(NON_ASCII) == 8
    assert unflat(sizes, data) == vals
    s0, d0, t0 = flat(coalesce_ref([None, None], b""))                              # all missing with "": two empty strings, no bytes
    assert s0.tolist() == [0, 0] and len(d0) == 0 and t0 == 0
    s1, d1, t1 = flat(coalesce_ref([None, None], [None, None]))
    assert s1.tolist() == [-1, -1] and t1 == 0


def test_the_case_table_holds_what_it_claims():
    rows = K.row_strings()
    assert len(rows) == K.N == 3 * 1024 + 37
    assert {len(r) for r in rows} == set(K.LENGTHS)
    assert all(r == b"" for r in rows[1024:2048]) and any(r for r in rows[:1024]) and any(r for r in rows[2048:])
    assert any(b"\0" in r for r in rows) and any(max(r, default=0) >= 0x80 for r in rows)
    starts = np.concatenate(([0], np.cumsum([len(r) for r in rows])[:-1]))
    assert {int(s) % 8 for s in starts[:1024]} == set(range(8))                      # a row starts on every byte alignment
    pats = K.missing_patterns()
    assert set(pats) == {"none", "all", "every7th", "first", "last", "tile2", "run-over-boundary"}
    assert pats["first"].sum() == 1 and pats["first"][0] and pats["last"].sum() == 1 and pats["last"][-1]
    assert pats["tile2"][2048:3072].all() and pats["tile2"].sum() == 1024
    r = pats["run-over-boundary"]
    assert r[1023] and r[1024] and not r[0] and r.sum() == 140
    plain, nullable = K.default_columns()
    assert all(v is not None for v in plain) and plain != rows
    miss_b = np.array([v is None for v in nullable])
    for name in ("all", "every7th", "tile2", "run-over-boundary"):
        assert (pats[name] & miss_b).any() and (pats[name] & ~miss_b).any(), name    # missing in both on some rows, filled from b on others
    assert [len(c) for c in K.CONSTANTS[:7]] == [0, 1, 7, 8, 9, 17, 40] and max(K.CONSTANTS[7]) >= 0x80


def test_ir_bytes_of_coalesce_and_string():
    from dfdb import ir
    col3 = struct.pack("<BI", 0x01, 3)
    assert ir.coalesce(ir.col(3), "x").to_ir() == col3 + struct.pack("<BI", 0x03, 1) + b"x" + b"\x45"
    assert ir.coalesce(ir.col(3), NON_ASCII).to_ir() == col3 + struct.pack("<BI", 0x03, len(NON_ASCII)) + NON_ASCII + b"\x45"
    assert ir.coalesce(ir.col(3), ir.col(0)).to_ir() == col3 + struct.pack("<BI", 0x01, 0) + b"\x45"
    assert ir.string(ir.col(3)).to_ir() == col3 + struct.pack("<BI", 0x03, 7) + b"missing" + b"\x45"      # string(missing) == "missing"
    assert ir.string(ir.col(3)).same(ir.coalesce(ir.col(3), "missing"))
    assert ir.string(ir.col(3), nullable=False).to_ir() == col3                                             # a plain String column: the column itself


def test_the_package_exports_string():
    import dfdb
    assert "string" in dfdb.__all__ and callable(dfdb.string)
    from dfdb import ir
    e = dfdb.string(ir.col(1))                                                       # an Expr carries no type: taken as nullable
    assert isinstance(e, ir.Expr) and e.same(ir.coalesce(ir.col(1), "missing"))
