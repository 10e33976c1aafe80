"""dfdb_sort_indices (csrc/k_sort.hip: a stable least-significant-digit radix sort of {key, row} pairs over a selection) and dfdb_gather_rows, against the
numpy restatement of tests/sort_cases.py.  Every comparison is exact: the table rows in their order, the pairs sorted (info[1]), the digit passes run and
skipped (info[2], info[3]), the gathered values bit for bit, and — after the calls — dfdb_count and dfdb_select_indices of the same query.  Row counts lie
around a 64-row bitmap word, a 1024-row tile, a 4096-row ctile, the sort's chunk of pairs (dfdb_selftest "sort_geometry") and 70 001: past one 65 536-row
block, several workgroups, a partial last word."""
import ctypes as C

import numpy as np
import pytest

import order_stat_cases as K
import sort_cases as S

pytestmark = pytest.mark.gpu


def add_raw(dfdb, t, name, values, missing=None):
    """a column exactly as given: the bytes under a missing flag stay what they are (DFTable.add_column zero-fills a masked array)"""
    from dfdb import _native as N, ir
    arr = np.ascontiguousarray(values)
    dt = ir.dtype_of_numpy(arr.dtype)
    m = None if missing is None else np.ascontiguousarray(missing, np.uint8)
    N.check(N.load().dfdb_table_add_column(t._h, name.encode(), dt | (ir.NULLABLE if m is not None else 0), len(arr), arr.ctypes.data if len(arr) else None, None, 0,
                                           m.ctypes.data if m is not None else None))


def one_column(dfdb, ctx, values, missing=None):
    t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    add_raw(dfdb, t, "x", values, missing)
    return t


def chunk_pairs():
    from dfdb import _native as N
    out = (C.c_int64 * 2)()
    N.check(N.load().dfdb_selftest(b"sort_geometry", 0, out, 2))
    return int(out[0])


def check_sort(col, values, missing=None, rows=None, limits=(None,), revs=(False, True), case=None):
    """col: the DFColumn of `values` under a selection that keeps the 0-based `rows` (None: all); `case` names the loop's case in a failure"""
    q = col.view._query()
    count0, idx0 = q.count(), q.indices().copy()
    assert np.array_equal(idx0, (np.arange(len(values)) if rows is None else np.asarray(rows)) + 1)
    for rev in revs:
        full = S.sortperm_ref(values, missing, rows, rev)
        for limit in limits:
            got, info = q.sort_indices(0, rev, limit)
            want = S.sortperm_ref(values, missing, rows, rev, limit)
            assert np.array_equal(want, full[:len(want)])
            assert got.dtype == np.int64 and np.array_equal(got, want), (case, rev, limit, got[:8], want[:8])
            assert info[0] == count0 and info[1] == S.candidates_ref(values, missing, rows, rev, limit), (case, rev, limit, info)
            assert (info[2], info[3]) == S.passes_ref(values, missing, rows, rev, limit), (case, rev, limit, info)
    assert q.count() == count0 and np.array_equal(q.indices(), idx0)      # the selection is as it was found


def test_row_counts(dfdb_mod, ctx):
    c = chunk_pairs()
    for kind in ("f64", "i32"):
        for n in K.ROW_COUNTS + (c - 1, c, c + 1, 3 * c + 17):
            x = K.rowcount_column(kind, n)
            t = one_column(dfdb_mod, ctx, x)
            check_sort(t[dfdb_mod.ALL, "x"], x, case=(kind, n))
            t.close()


def test_value_shapes_and_pass_skipping(dfdb_mod, ctx):
    for shape in K.SHAPES:
        for n in K.SHAPE_ROWS:
            x = K.shape_column(shape, n)
            t = one_column(dfdb_mod, ctx, x)
            check_sort(t[dfdb_mod.ALL, "x"], x, case=(shape, n))
            if shape in ("equal", "low_byte", "high_byte"):
                _, info = t[dfdb_mod.ALL, "x"].view._query().sort_indices(0)
                assert info[2:] == ((0, 8) if shape == "equal" else (1, 7)), (shape, n, info)
            t.close()


def test_small_int64_values_take_three_passes(dfdb_mod, ctx):
    t = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    t.add_generated("x", dfdb_mod.GEN_I64_MOD1M, 7, 70_001)
    col = t[dfdb_mod.ALL, "x"]
    x = dfdb_mod.materialize(col)
    assert x.dtype == np.int64 and x.min() >= 0 and x.max() < 1_000_000
    got, info = col.view._query().sort_indices(0)
    assert np.array_equal(got, S.sortperm_ref(x)) and info == (70_001, 70_001, 3, 5)


def test_selections(dfdb_mod, ctx):
    x, u, tt = K.selection_table()
    t = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    for name, v in (("x", x), ("u", u), ("t", tt)):
        add_raw(dfdb_mod, t, name, v)
    sels = K.selections(u, tt)
    for name in ("none", "range", "indices", "pred10", "nothing", "empty_tiles"):
        spec, rows = sels[name]
        if spec is None:
            col = t[dfdb_mod.ALL, "x"]
        elif spec[0] == "range":
            col = t[dfdb_mod.jr(spec[1], spec[2], dfdb_mod.END), "x"]
        elif spec[0] == "indices":
            col = t[list(spec[1]), "x"]
        else:
            k = spec[3]
            col = t[(spec[1], (lambda c: c < k) if spec[2] == "<" else (lambda c: c == k)), "x"]
        check_sort(col, x, rows=rows, limits=(None, 10), case=name)
    t.close()


def tie_columns(n):
    rng = np.random.default_rng(n)
    one_off = np.full(n, 7, np.int64)
    one_off[n // 2] = 3
    return {"bool": rng.random(n) < 0.3, "u%3": (rng.integers(0, 100, n) % 3).astype(np.int64), "one_off": one_off}


def test_ties_keep_row_order_in_both_directions(dfdb_mod, ctx):
    n = 3 * chunk_pairs() + 17
    for name, x in tie_columns(n).items():
        t = one_column(dfdb_mod, ctx, x)
        check_sort(t[dfdb_mod.ALL, "x"], x, case=name)
        check_sort(t[dfdb_mod.jr(2, 3, dfdb_mod.END), "x"], x, rows=np.arange(1, n, 3), case=name)
        t.close()


def test_nullable_garbage_never_moves_a_row(dfdb_mod, ctx):
    for n in K.SHAPE_ROWS:
        x, m = K.nullable_column(n)
        t = one_column(dfdb_mod, ctx, x, m)
        check_sort(t[dfdb_mod.ALL, "x"], x, m, case=n)
        check_sort(t[dfdb_mod.jr(1, 7, dfdb_mod.END), "x"], x, m, rows=np.arange(0, n, 7), case=n)
        check_sort(t[dfdb_mod.jr(7, 7, dfdb_mod.END), "x"], x, m, rows=np.arange(6, n, 7), limits=(None, 3), case=n)     # the missing rows alone
        i = (np.arange(n) * 37 % 251 - 125).astype(np.int8)                                         # a narrow nullable column: garbage 127 / -128 under the flags
        i[m] = np.where(np.arange(int(m.sum())) % 2 == 0, 127, -128).astype(np.int8)
        t2 = one_column(dfdb_mod, ctx, i, m)
        check_sort(t2[dfdb_mod.ALL, "x"], i, m, case=n)
        t.close()
        t2.close()


def test_all_rows_missing(dfdb_mod, ctx):
    x, m = K.nullable_column(1025, all_missing=True)
    t = one_column(dfdb_mod, ctx, x, m)
    check_sort(t[dfdb_mod.ALL, "x"], x, m, limits=(None, 0, 5))
    got, info = t[dfdb_mod.ALL, "x"].view._query().sort_indices(0, True)
    assert np.array_equal(got, np.arange(1, 1026)) and info == (1025, 0, 0, 8)


def test_limit_is_the_prefix_and_sorts_only_the_candidates(dfdb_mod, ctx):
    n = 3 * chunk_pairs() + 17
    for name in ("random", "ties", "nullable"):
        m = None
        if name == "random":
            x = K.rowcount_column("f64", n)
        elif name == "ties":
            x = tie_columns(n)["u%3"]
        else:
            x, m = K.nullable_column(n)
        t = one_column(dfdb_mod, ctx, x, m)
        check_sort(t[dfdb_mod.ALL, "x"], x, m, limits=(0, 1, 2, 10, n - 1, n, n + 5), case=name)
        if name == "random":
            _, info = t[dfdb_mod.ALL, "x"].view._query().sort_indices(0, False, 10)
            assert info[1] < 100                                                                    # a top-10 of distinct values sorts a handful of pairs
        t.close()


def test_device_output_feeds_gather_rows_and_calls_repeat(dfdb_mod, ctx):
    import torch
    n = chunk_pairs() + 1
    x = K.rowcount_column("f64", n)
    t = one_column(dfdb_mod, ctx, x)
    q = t[dfdb_mod.ALL, "x"].view._query()
    want = S.sortperm_ref(x, rev=True)
    buf = torch.full((n + 2,), -7, dtype=torch.int64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()                # (the fill runs on torch's stream, the sort on the engine's own: order them)
    none, info = q.sort_indices(0, True, None, dev_ptr=buf.data_ptr() + 8, cap=n)                   # device memory, n = NULL
    ctx.synchronize()
    h = buf.cpu().numpy()
    assert none is None and info[0] == n and h[0] == -7 and h[-1] == -7 and np.array_equal(h[1:-1], want)
    vals = q.gather_rows(dev_ptr=buf.data_ptr() + 8, n=n)[0]                                        # the rows never leave the device
    assert np.array_equal(K.bits_of(vals), K.bits_of(x[want - 1]))
    buf.fill_(-7)
    torch.cuda.synchronize()
    q.sort_indices(0, True, None, dev_ptr=buf.data_ptr(), cap=5)                                    # a capacity below the count: nothing beyond it is written
    ctx.synchronize()
    h = buf.cpu().numpy()
    assert np.array_equal(h[:5], want[:5]) and np.all(h[5:] == -7)
    a, ia = q.sort_indices(0, False)
    b, ib = q.sort_indices(0, False)                                                                # two calls in a row
    assert np.array_equal(a, b) and ia == ib and np.array_equal(a, S.sortperm_ref(x))
    t.close()


@pytest.fixture(scope="module")
def wide_table(dfdb_mod, ctx):
    n = 5000
    rng = np.random.default_rng(5000)
    cols = {"b": rng.integers(-128, 128, n).astype(np.int8), "h": rng.integers(0, 65536, n).astype(np.uint16), "f": rng.standard_normal(n).astype(np.float32),
            "d": rng.standard_normal(n), "z": rng.integers(-5, 5, n).astype(np.int64)}
    zm = rng.random(n) < 0.2
    t = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    for name, v in cols.items():
        add_raw(dfdb_mod, t, name, v, zm if name == "z" else None)
    return t, cols, zm


def check_gather(q, names, cols, zm, rows):
    got = q.gather_rows(rows)
    assert len(got) == len(names)
    idx = np.asarray(rows, np.int64) - 1
    for name, g in zip(names, got):
        assert len(g) == len(idx) and g.dtype == cols[name].dtype
        if name == "z":
            assert isinstance(g, np.ma.MaskedArray) and np.array_equal(np.ma.getmaskarray(g), zm[idx])
            assert np.array_equal(np.asarray(g.data)[~zm[idx]], cols[name][idx][~zm[idx]])
        else:
            assert np.array_equal(K.bits_of(g), K.bits_of(cols[name][idx]))


def test_gather_rows_follows_any_row_order(dfdb_mod, ctx, wide_table):
    t, cols, zm = wide_table
    names = list(cols)
    v = t[("h", lambda h: h < 30000), dfdb_mod.ALL]                                                 # the gather does not depend on the selection
    q = v._query()
    assert list(v.projection.keys()) == names
    n = len(cols["d"])
    for by in ("d", "z"):
        rows, _ = q.sort_indices(names.index(by), True)
        sel = np.flatnonzero(cols["h"] < 30000)
        assert np.array_equal(rows, S.sortperm_ref(cols[by], zm if by == "z" else None, sel, True))
        check_gather(q, names, cols, zm, rows)
    check_gather(q, names, cols, zm, [n, 1, 1, 4097, 2, n, 1024, 1025, 1, 64])                      # a hand permutation with repeats, selected or not
    check_gather(q, names, cols, zm, [])
    for bad in (0, n + 1, -3):
        with pytest.raises(IndexError):
            q.gather_rows([1, bad, 2])
    assert q.count() == int((cols["h"] < 30000).sum())


def test_refusals_name_the_form(dfdb_mod, ctx):
    x = (np.arange(70_001, dtype=np.int64) * 7919) % 10_007
    t = one_column(dfdb_mod, ctx, x)
    t.add_column("s", ["a", "b", "c"] * 23_333 + ["a", "b"])
    for call in (lambda c: c.view._query().sort_indices(0), lambda c: c.view._query().gather_rows([1])):
        with pytest.raises(NotImplementedError, match="String"):
            call(t[dfdb_mod.ALL, "s"])
        with pytest.raises(NotImplementedError, match="computed column"):
            call(t[dfdb_mod.ALL, "x"] + 1)
    q = t[dfdb_mod.ALL, "x"].view._query()
    for bad in (1, -1):
        with pytest.raises(IndexError):
            q.sort_indices(bad)
    from dfdb import _native as N
    with pytest.raises(ValueError):
        N.check(N.load().dfdb_sort_indices(q._h, 0, 2, -1, None, 0, N.MEM_HOST, None, None))        # a flag that does not exist
    assert np.array_equal(q.sort_indices(0)[0], S.sortperm_ref(x))
    t.compress_column("x", 2)                                                                       # what keep_compressed = 2 leaves: the LZ4 blocks alone
    assert t.resident_bytes("x")["decoded"] == 0
    with pytest.raises(NotImplementedError, match="compressed-only"):
        t[dfdb_mod.ALL, "x"].view._query().sort_indices(0)
    with pytest.raises(NotImplementedError, match="compressed-only"):
        t[dfdb_mod.ALL, "x"].view._query().gather_rows([1])
    assert dfdb_mod.nrow(t[dfdb_mod.ALL, "x"]) == len(x)                                            # (the column still answers what it answered)


def test_python_api_agrees_with_the_raw_calls(dfdb_mod, ctx, wide_table):
    t, cols, zm = wide_table
    d = t[("h", lambda h: h < 30000), "d"]
    sel = np.flatnonzero(cols["h"] < 30000)
    for rev in (False, True):
        want = S.sortperm_ref(cols["d"], None, sel, rev)
        assert np.array_equal(d.sortperm(rev=rev), want) and np.array_equal(dfdb_mod.sortperm(d, rev=rev), want)
        assert np.array_equal(d.sortperm(rev=rev, limit=10), want[:10]) and np.array_equal(dfdb_mod.partialsortperm(d, 10, rev=rev), want[:10])
        assert np.array_equal(K.bits_of(d.sort(rev=rev)), K.bits_of(cols["d"][want - 1]))
        assert np.array_equal(K.bits_of(dfdb_mod.sort(d, rev=rev, limit=7)), K.bits_of(cols["d"][want[:7] - 1]))
    z = t[dfdb_mod.ALL, "z"]
    want = S.sortperm_ref(cols["z"], zm, None, True)
    got = z.sort(rev=True)
    assert isinstance(got, np.ma.MaskedArray) and np.array_equal(np.ma.getmaskarray(got), zm[want - 1])
    assert np.array_equal(got.compressed(), cols["z"][want - 1][~zm[want - 1]])
    v = t[("h", lambda h: h < 30000), ["d", "b", "f"]]
    df = dfdb_mod.sort_view(v, "b", rev=False, limit=100)
    want = S.sortperm_ref(cols["b"], None, sel, False, 100)
    assert list(df.columns) == ["d", "b", "f"] and len(df) == 100
    for name in ("d", "b", "f"):
        assert np.array_equal(K.bits_of(df[name].to_numpy()), K.bits_of(cols[name][want - 1]))
