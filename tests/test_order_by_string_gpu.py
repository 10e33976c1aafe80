"""dfdb_sort_indices_any (csrc/sort.cpp: a String key run as its m + 1 eight-byte sub-keys — length, then chunk m-1 .. chunk 0 — through the sort driver,
keyed by k_sort_strkey of csrc/k_sort.hip) against the restatement of tests/sort_str_cases.py.  Every comparison is exact: the table rows in their order and
info (selected rows, pairs keyed, digit passes run and skipped, summed over keys and sub-keys); after the calls dfdb_count of the same query.  String lengths
lie around the 8-byte chunk (0, 1, 7, 8, 9, 15, 16, 17) and at the cap (255, 256); row counts around a 64-row word, a 1024-entry wave span of the order, a
1024-row tile of the column, the sort's 4096-pair chunk and 70 001 (several workgroups, a partial last word).  Every test makes its own tables, sets no
context option and leaves the session's context as it found it: the file passes alone, in front of the other GPU tests and behind them."""
import ctypes as C
import os
import shutil
import tempfile

import numpy as np
import pytest

import order_stat_cases as K
import sort_str_cases as T

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4097, 70_001)
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 255, 256)


class Cols:
    """a table of String columns (lists of bytes / None) and raw numeric columns (array, or (array, missing flags)), and what the restatement needs of them"""

    def __init__(self, dfdb, ctx, cols, nullable=()):
        from dfdb import _native as N, ir
        self.dfdb, self.names, self.values, self.missing = dfdb, list(cols), [], []
        self.t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
        for name, v in cols.items():
            if T.is_string_key(v):
                self.values.append(list(v)); self.missing.append(None)
                self.t.add_column(name, list(v), dtype=ir.STRING | ir.NULLABLE if name in nullable else None)
                continue
            arr = np.ascontiguousarray(v[0] if isinstance(v, tuple) else v)
            m = np.ascontiguousarray(v[1], np.uint8) if isinstance(v, tuple) else None
            self.values.append(arr); self.missing.append(m)
            N.check(N.load().dfdb_table_add_column(self.t._h, name.encode(), ir.dtype_of_numpy(arr.dtype) | (ir.NULLABLE if m is not None else 0), len(arr),
                                                   arr.ctypes.data if len(arr) else None, None, 0, m.ctypes.data if m is not None else None))

    def query(self, selector=None):
        return self.t[self.dfdb.ALL if selector is None else selector, self.dfdb.ALL]._query()

    def keys(self, names):
        idx = [self.names.index(k) for k in names]
        return idx, [self.values[i] for i in idx], [self.missing[i] for i in idx]

    def check(self, names, revs, q=None, rows=None, limits=(None,), case=None):
        """the call by the columns `names` (major first) on query q (default: no selection; `rows`: the 0-based rows q keeps) against the restatement"""
        q = self.query() if q is None else q
        idx, kc, km = self.keys(names)
        count0 = q.count()
        assert count0 == (len(kc[0]) if rows is None else len(rows))
        full, winfo = T.sortperm_any_ref(kc, km, rows, revs), T.info_any_ref(kc, km, rows, revs)
        for limit in limits:
            got, info = q.sort_indices_any(idx, revs, limit)
            want = full if limit is None else full[:limit]
            assert got.dtype == np.int64 and np.array_equal(got, want), (case, names, revs, limit, got[:8], want[:8])
            assert info == winfo, (case, names, revs, limit, info, winfo)
        assert q.count() == count0                      # the selection is as it was found

    def close(self):
        self.t.close()


def edge_pool():
    """strings of every length of LENGTHS, sharing their first 8 / 16 bytes, tying on every chunk and differing in length (trailing NULs), with embedded
    NULs and bytes >= 0x80, multi-byte UTF-8"""
    pool = [b"", b"a", b"b", b"\0", b"\0\0", b"a\0", b"a\0\0", b"a\0b", b"abcdefg", b"abcdefgh", b"abcdefgh\0", b"abcdefghi", b"abcdefghj", b"abcdefg\0",
            b"abcdefg\0\0", b"abcdefghabcdefg", b"abcdefghabcdefgh", b"abcdefghabcdefgh\0", b"abcdefghabcdefghi", b"abcdefghabcdefgi", b"abcdefghabcdefgh\xff",
            "é".encode(), "z".encode(), "日本".encode(), "日本語".encode(), "日本語のテキスト".encode(), b"\x7f", b"\x80", b"\xff" * 9, b"\xff" * 8]
    base = bytes((i * 37 + 11) % 251 + 1 for i in range(256))
    pool += [base[:n] for n in LENGTHS] + [base[:254] + b"\0", base[:255] + b"\0", base[:255] + b"\1", base[:248] + b"\0" * 8, base[:248] + b"\0" * 7]
    assert {len(p) for p in pool} >= set(LENGTHS) and max(len(p) for p in pool) == 256
    return pool


def short_pool():
    return [b"", b"a", b"ab", b"a\0", b"abcdefg", b"abcdefgh", b"abcdefgh\0", b"abcdefghi", b"abcdefghij", "é".encode(), b"z", b"0123456789abcdef", b"0123456789abcdefX",
            b"0123456789abcdeg", b"01234567", b"0123456", b"brand-7", b"brand-70", b"brand-8"]


def draw(pool, n, seed, missing_every=0):
    rng = np.random.default_rng([n, seed])
    v = [pool[i] for i in rng.integers(0, len(pool), n)]
    if missing_every:
        for i in range(missing_every - 2, n, missing_every):
            v[i] = None
    return v


def test_lengths_around_the_chunk_and_at_the_cap(dfdb_mod, ctx):
    n = 1025
    T_ = Cols(dfdb_mod, ctx, {"e": draw(edge_pool(), n, 1), "equal": [b"samsung"] * n, "empty": [b""] * n, "i": K.rowcount_column("i32", n)})
    q = T_.query()
    for rev in (False, True):
        T_.check(["e"], [rev], q=q, case="edge")
        T_.check(["equal"], [rev], q=q, case="equal")                # one chunk and the length: every pass of the two sub-keys is skipped
        T_.check(["empty"], [rev], q=q, case="empty")                # m = 0: the length alone
    assert q.sort_indices_any([1])[1] == (n, 2 * n, 0, 16) and q.sort_indices_any([2])[1] == (n, n, 0, 8)
    assert np.array_equal(q.sort_indices_any([1], [True])[0], np.arange(1, n + 1))
    T_.check(["equal", "i"], [False, True], q=q)
    T_.close()


def test_row_counts(dfdb_mod, ctx):
    for n in ROW_COUNTS:
        T_ = Cols(dfdb_mod, ctx, {"s": draw(short_pool(), n, 2), "x": K.rowcount_column("i32", n).astype(np.int64)})
        q = T_.query()
        for rev in (False, True):
            T_.check(["s"], [rev], q=q, case=n)
        T_.check(["s", "x"], [True, False], q=q, case=n)
        T_.close()


def test_missing_rows_a_fifth_and_a_whole_tile(dfdb_mod, ctx):
    n = 4097
    fifth = draw(short_pool(), n, 3, missing_every=5)
    tile = draw(short_pool(), n, 4)
    tile[1024:2048] = [None] * 1024
    none = [None] * n
    T_ = Cols(dfdb_mod, ctx, {"fifth": fifth, "tile": tile, "none": none, "plain": draw(short_pool(), n, 5), "i": K.rowcount_column("i32", n)}, nullable=("plain",))
    q = T_.query()
    for rev in (False, True):
        for name in ("fifth", "tile", "none", "plain"):
            T_.check([name], [rev], q=q, case=name)
        T_.check(["fifth", "tile"], [rev, not rev], q=q)
        T_.check(["tile", "i"], [rev, False], q=q)
        T_.check(["i", "fifth"], [False, rev], q=q)
    T_.close()


def test_selections_and_the_over_long_string_outside_them(dfdb_mod, ctx):
    n = 4097                                                           # (70 001 rows: test_row_counts; here what matters is which rows are selected)
    rng = np.random.default_rng([n, 15])
    x, u, tt = rng.standard_normal(n) * 1000.0, rng.integers(0, 100, n).astype(np.int64), (np.arange(n) // 300).astype(np.int64)
    s = draw(short_pool(), n, 6, missing_every=7)
    long_row = int(np.flatnonzero(u >= 90)[0])
    s[long_row] = b"L" * 257                                           # the only over-long string: outside u < 90
    T_ = Cols(dfdb_mod, ctx, {"x": x, "u": u, "t": tt, "s": s, "p": draw(short_pool(), n, 8)})
    idx = np.sort(rng.choice(n, 333, replace=False))
    sels = {"none": (None, np.arange(n)), "range": (dfdb_mod.jr(1, 7, dfdb_mod.END), np.arange(0, n, 7)), "indices": ((idx + 1).tolist(), idx),
            "pred10": (("u", lambda c: c < 10), np.flatnonzero(u < 10)), "pred90": (("u", lambda c: c < 90), np.flatnonzero(u < 90)),
            "nothing": (("u", lambda c: c < 0), np.zeros(0, np.int64)),
            "empty_tiles": (("t", lambda c: c == 5), np.flatnonzero(tt == 5))}      # rows 1500 .. 1799: three of the five 1024-row tiles are empty
    answered = 0
    for name, (sel, rows) in sels.items():
        q = T_.query(sel)
        T_.check(["p"], [False], q=q, rows=rows, limits=(None, 10), case=name)
        T_.check(["u", "p", "x"], [True, False, False], q=q, rows=rows, case=name)
        if long_row not in set(rows.tolist()):
            T_.check(["s"], [True], q=q, rows=rows, case=name)        # the over-long row is not selected: answered
            T_.check(["x", "s"], [False, False], q=q, rows=rows, case=name)
            answered += 1
    assert answered >= 3 and long_row not in set(sels["pred90"][1].tolist())
    T_.close()


def test_key_positions(dfdb_mod, ctx):
    n = 4097
    rng = np.random.default_rng(n)
    i32 = rng.integers(-3, 3, n).astype(np.int32)
    im = rng.random(n) < 0.2
    i32[im] = np.where(np.arange(int(im.sum())) % 2 == 0, 2**31 - 1, -2**31).astype(np.int32)      # garbage under the flags
    T_ = Cols(dfdb_mod, ctx, {"s": draw(short_pool(), n, 9, missing_every=5), "e": draw(edge_pool(), n, 10), "x": rng.integers(0, 50, n).astype(np.int64),
                              "ni": (i32, im), "few": draw([b"apple", b"samsung", b"xiaomi"], n, 11)})
    q = T_.query()
    for revs in ((False, False), (False, True), (True, False), (True, True)):
        T_.check(["few", "x"], revs, q=q)                             # major over an Int64 minor
        T_.check(["ni", "s"], revs, q=q)                              # minor under a nullable Int32 major
        T_.check(["few", "s"], revs, q=q)                             # two String keys
    T_.check(["s", "s"], [False, True], q=q)                          # the same String column twice, opposite rev
    T_.check(["s", "s"], [True, False], q=q)
    T_.check(["few", "e", "x"], [True, False, True], q=q)
    T_.check(["x", "few", "ni", "s"], [False, True, False, True], q=q)
    T_.close()


def test_limit_is_the_prefix(dfdb_mod, ctx):
    n = 4097
    T_ = Cols(dfdb_mod, ctx, {"s": draw(short_pool(), n, 12, missing_every=5), "x": K.rowcount_column("i32", n).astype(np.int64)})
    q = T_.query()
    limits = (0, 1, 10, n, n + 5)
    for rev in (False, True):
        T_.check(["s"], [rev], q=q, limits=limits)
    T_.check(["s", "x"], [True, False], q=q, limits=limits)
    rows = np.arange(2, n, 3)
    T_.check(["s"], [True], q=T_.query(dfdb_mod.jr(3, 3, dfdb_mod.END)), rows=rows, limits=(0, 1, 10, len(rows), len(rows) + 5))
    T_.close()


def test_device_output_feeds_gather_rows_any(dfdb_mod, ctx):
    import torch
    n = 4097
    s = draw(short_pool(), n, 13, missing_every=5)
    T_ = Cols(dfdb_mod, ctx, {"s": s, "x": K.rowcount_column("i32", n).astype(np.int64)})
    q = T_.query()
    want = T.sortperm_any_ref([s], [None], None, [True])
    buf = torch.full((n + 2,), -7, dtype=torch.int64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()                # (the fill runs on torch's stream, the sort on the engine's own: order them)
    none, info = q.sort_indices_any([0], [True], None, dev_ptr=buf.data_ptr() + 8, cap=n)
    ctx.synchronize()
    h = buf.cpu().numpy()
    assert none is None and info == T.info_any_ref([s], [None], None, [True]) and h[0] == -7 and h[-1] == -7 and np.array_equal(h[1:-1], want)
    sizes, data = q.gather_rows_any(dev_ptr=buf.data_ptr() + 8, n=n)[0]                              # the rows never leave the device
    ordered = [s[r - 1] for r in want]
    assert np.array_equal(sizes, [-1 if v is None else len(v) for v in ordered]) and data.tobytes() == b"".join(v for v in ordered if v)
    buf.fill_(-7)
    torch.cuda.synchronize()
    q.sort_indices_any([0], [True], None, dev_ptr=buf.data_ptr(), cap=5)                             # a capacity below the count: nothing beyond it is written
    ctx.synchronize()
    h = buf.cpu().numpy()
    assert np.array_equal(h[:5], want[:5]) and np.all(h[5:] == -7)
    T_.close()


def test_a_column_with_a_dictionary_and_numeric_keys_alone(dfdb_mod, ctx):
    n = 2049
    brands = [b"apple", b"", b"samsung", b"xiaomi", "é".encode(), b"a-much-longer-brand-name"]
    T_ = Cols(dfdb_mod, ctx, {"b": [brands[(i * 7) % len(brands)] for i in range(n)], "x": K.rowcount_column("i32", n).astype(np.int64), "f": K.nullable_column(n),
                              "g": (np.arange(n) % 3).astype(np.int8)})
    q = T_.query()
    before = [q.sort_indices_any([0], [rev]) for rev in (False, True)]
    assert T_.t.build_dictionary("b") == len(brands)
    for rev in (False, True):
        T_.check(["b"], [rev], q=q, case="dictionary")
        assert np.array_equal(q.sort_indices_any([0], [rev])[0], before[rev][0]) and q.sort_indices_any([0], [rev])[1] == before[rev][1]
    T_.check(["b", "x"], [True, False], q=q, case="dictionary")
    # numeric keys only: dfdb_sort_indices_n's answer and info, one key (the top-k cut) and several
    q2 = T_.query(dfdb_mod.jr(1, 2, dfdb_mod.END))
    for keys, revs in (([1], [False]), ([2], [True]), ([3, 2], [False, True]), ([3, 1, 2], [True, True, False])):
        for limit in (None, 0, 1, 10, n):
            a, ia = q2.sort_indices_n(keys, revs, limit)
            b, ib = q2.sort_indices_any(keys, revs, limit)
            assert np.array_equal(a, b) and ia == ib, (keys, revs, limit, ia, ib)
    T_.close()


def test_sort_view_and_the_column_sorts_against_pandas(dfdb_mod, ctx):
    import pandas as pd
    n = 2100                                                           # three tiles of the column, the last one partial
    rng = np.random.default_rng(n)
    words = ["", "a", "ab", "abcdefgh", "abcdefghi", "apple", "samsung", "xiaomi", "é", "日本語", "zz-top-of-the-ascii", "brand-7", "brand-70"]
    s = [None if i % 9 == 4 else words[j] for i, j in enumerate(rng.integers(0, len(words), n))]
    x = rng.integers(0, 40, n).astype(np.int64)
    t = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    t.add_column("s", s)
    t.add_column("x", x)
    v = t[("x", lambda c: c < 30), ["s", "x"]]
    keep = np.flatnonzero(x < 30)
    frame = pd.DataFrame({"s": np.array(s, object)[keep], "x": x[keep]})
    for by, rev, na in (("s", False, "last"), ("s", True, "first"), (["s", "x"], [True, False], "first"), (["x", "s"], [False, False], "last")):
        asc = [not r for r in rev] if isinstance(rev, list) else not rev
        want = frame.sort_values(by, ascending=asc, kind="stable", na_position=na)
        for limit in (None, 10):
            w = want if limit is None else want.head(limit)
            got = dfdb_mod.sort_view(v, by, rev=rev, limit=limit)
            assert list(got.columns) == ["s", "x"] and len(got) == len(w), (by, rev, limit)
            assert list(got["s"]) == list(w["s"]) and np.array_equal(got["x"].to_numpy(), w["x"].to_numpy()), (by, rev, limit)
    col = t[("x", lambda c: c < 30), "s"]
    enc = [None if e is None else e.encode() for e in s]
    for rev in (False, True):
        want = T.sortperm_any_ref([enc], [None], keep, [rev])
        assert np.array_equal(col.sortperm(rev=rev), want) and np.array_equal(dfdb_mod.sortperm(col, rev, 7), want[:7])
        assert np.array_equal(dfdb_mod.sortperm_by(v, ["s", "x"], rev=[rev, False]), T.sortperm_any_ref([enc, x], [None, None], keep, [rev, False]))
        assert list(col.sort(rev=rev)) == [s[r - 1] for r in want] and list(dfdb_mod.sort(col, rev, 7)) == [s[r - 1] for r in want[:7]]
    t.close()


def test_refusals_name_the_column_or_the_form(dfdb_mod, ctx):
    import torch
    from dfdb import _native as N
    n = 3000
    x = (np.arange(n, dtype=np.int64) * 7919) % 10_007
    s = draw(short_pool(), n, 14)
    s[1500] = b"L" * 257
    T_ = Cols(dfdb_mod, ctx, {"x": x, "s": s})
    t = T_.t
    q = T_.query()
    L = N.load()
    # a 257-byte live selected string: refused by name, with the length found and the limit; `out` stays as it was, in device and in host memory
    buf = torch.full((n,), -7, dtype=torch.int64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    for keys in ([1], [0, 1], [1, 0]):
        with pytest.raises(NotImplementedError, match=r"String column s .* 257 bytes.* 256"):
            q.sort_indices_any(keys, None, None, dev_ptr=buf.data_ptr(), cap=n)
        ctx.synchronize()
        assert bool((buf == -7).all())
        host = np.full(n, -7, np.int64)
        one, zero = (C.c_int32 * 2)(*(keys + [0])[:2]), (C.c_int32 * 2)()
        with pytest.raises(NotImplementedError, match="DFDB_SORT_MAX_STRING_BYTES"):
            N.check(L.dfdb_sort_indices_any(q._h, one, zero, len(keys), -1, host.ctypes.data, n, N.MEM_HOST, None, None))
        assert np.all(host == -7) and q.count() == n
    short = T_.query(dfdb_mod.jr(1, 1, 1500))                          # rows 1..1500: the long one is row 1501
    T_.check(["s"], [False], q=short, rows=np.arange(1500))
    # computed columns, a coalesce among them
    sc, xc = t[dfdb_mod.ALL, "s"], t[dfdb_mod.ALL, "x"]
    with pytest.raises(NotImplementedError, match="sorting by a computed column"):
        dfdb_mod.coalesce(sc, "none").view._query().sort_indices_any([0])
    with pytest.raises(NotImplementedError, match="sorting by a computed column"):
        dfdb_mod.view_from_columns(s=sc, y=xc + 1)._query().sort_indices_any([0, 1])
    # arguments: dfdb_sort_indices_n's messages
    for bad in ([0, 2], [-1, 0], [2]):
        with pytest.raises(IndexError):
            q.sort_indices_any(bad)
    two, one = (C.c_int32 * 9)(*([0, 1] + [0] * 7)), (C.c_int32 * 9)()
    for nkeys in (0, 9, -1):
        with pytest.raises(ValueError, match="sort keys"):
            N.check(L.dfdb_sort_indices_any(q._h, two, one, nkeys, -1, None, 0, N.MEM_HOST, None, None))
    with pytest.raises(ValueError):
        N.check(L.dfdb_sort_indices_any(q._h, None, one, 2, -1, None, 0, N.MEM_HOST, None, None))
    with pytest.raises(ValueError):
        N.check(L.dfdb_sort_indices_any(q._h, two, None, 2, -1, None, 0, N.MEM_HOST, None, None))
    for flags in ((2, 0), (0, 2), (1, 3)):
        with pytest.raises(ValueError, match="sort flags"):
            N.check(L.dfdb_sort_indices_any(q._h, two, (C.c_int32 * 2)(*flags), 2, -1, None, 0, N.MEM_HOST, None, None))
    # the old entry points refuse the same column as before, and the query answers as before
    with pytest.raises(NotImplementedError, match="sorting by a String column"):
        q.sort_indices(1)
    with pytest.raises(NotImplementedError, match="sorting by a String column"):
        q.sort_indices_n([0, 1])
    assert np.array_equal(q.sort_indices_any([0])[0], q.sort_indices(0)[0]) and q.count() == n
    # out of core: opened, not loaded
    d = tempfile.mkdtemp(prefix="dfdb_sortstr_")
    try:
        s2 = list(s)
        s2[1500] = b"fits"
        T2 = Cols(dfdb_mod, ctx, {"x": x, "s": s2})
        T2.t.save(os.path.join(d, "tb"))
        ooc = dfdb_mod.open_table(os.path.join(d, "tb"), ctx=ctx, load=False)
        with pytest.raises(NotImplementedError, match="out of core"):
            ooc[dfdb_mod.ALL, dfdb_mod.ALL]._query().sort_indices_any([1, 0])
        ooc.load()                                                                                  # loaded: answered
        assert np.array_equal(ooc[dfdb_mod.ALL, dfdb_mod.ALL]._query().sort_indices_any([1, 0])[0], T.sortperm_any_ref([s2, x], [None, None]))
        ooc.close()
        T2.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    T_.close()
    big = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)             # one 4 MiB string: the tile limit's message, before any launch
    big.add_column("big", ["x" * (4 << 20)])
    qb = big[dfdb_mod.ALL, ["big"]]._query()
    with pytest.raises(NotImplementedError, match="String column big"):
        qb.sort_indices_any([0])
    assert qb.count() == 1
    big.close()
