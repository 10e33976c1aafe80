"""dfdb_order_statistics (csrc/k_select.hip: radix select over a selection) and DFColumn.median / quantile on top of it, against the numpy restatement of
tests/order_stat_cases.py.  Every comparison is exact: the 64 bits of every value (a NaN must also be the canonical quiet NaN), the three counts, and —
after the calls — dfdb_count and dfdb_select_indices of the same query.  Every case runs twice: with the select key in the column's own width (the
default: the passes over image bits that carry no order are skipped) and with ctx option "select_full_image" = 1 (the whole 64-bit order image, 8 passes);
the answers must not differ.  Row counts: around a 64-row bitmap word, a 1024-row tile, a 4096-row ctile, and 70 001 — past one 65 536-row block, 69
tiles over several workgroups, a partial last word."""
import ctypes as C
import os
import shutil
import tempfile

import numpy as np
import pytest

import order_stat_cases as K

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


def ranks16(n, seed):
    """16 ranks of 1..n in no order, with repeats, the ends and the middles among them"""
    rng = np.random.default_rng(seed)
    r = np.concatenate([[n, 1, (1 + n) // 2, n // 2 + 1, n, 1], rng.integers(1, n + 1, 10)])
    rng.shuffle(r)
    return r.astype(np.int64)


def check_column(ctx, col, values, missing=None, rows=None):
    """col: the DFColumn of `values` under a selection that keeps the 0-based `rows` (None: all)"""
    want, cnt = K.ordered(values, missing, rows), K.counts(values, missing, rows)
    n = cnt[0]
    q = col.view._query()
    count0, idx0 = q.count(), q.indices().copy()
    assert count0 == n + cnt[1] and np.array_equal(idx0, (np.arange(len(values)) if rows is None else np.asarray(rows)) + 1)
    for full in (0, 1):
        ctx.set_option("select_full_image", full)
        try:
            v, c = q.order_statistics([])                                  # nranks = 0: the counts alone
            assert len(v) == 0 and c == cnt, (full, c, cnt)
            if n == 0:
                with pytest.raises(IndexError):
                    q.order_statistics([1])
                continue
            single = {}
            for r in sorted({1, n, (1 + n) // 2, n // 2 + 1}):             # the ends and the two middles, one per call
                v, c = q.order_statistics([r])
                assert c == cnt and len(v) == 1
                assert K.bits_of(v)[0] == K.bits_of(want[r - 1:r])[0], (full, r, v, want[r - 1])
                single[r] = K.bits_of(v)[0]
            r16 = ranks16(n, n + full)
            v, c = q.order_statistics(r16)                                 # 16 in one call, unsorted, with repeats
            assert c == cnt and np.array_equal(K.bits_of(v), K.bits_of(want[r16 - 1])), (full, r16, v)
            assert all(K.bits_of(v)[k] == single[int(r)] for k, r in enumerate(r16) if int(r) in single)
            for bad in (0, n + 1, -1):
                with pytest.raises(IndexError):
                    q.order_statistics([1, bad])
        finally:
            ctx.set_option("select_full_image", 0)
    assert q.count() == count0 and np.array_equal(q.indices(), idx0)      # the selection is as it was found


@pytest.mark.parametrize("kind", ["f64", "i32"])
def test_row_counts(dfdb_mod, ctx, kind):
    for n in K.ROW_COUNTS:
        x = K.rowcount_column(kind, n)
        t = one_column(dfdb_mod, ctx, x)
        check_column(ctx, t[dfdb_mod.ALL, "x"], x)
        t.close()


@pytest.mark.parametrize("shape", K.SHAPES)
def test_value_shapes(dfdb_mod, ctx, shape):
    for n in K.SHAPE_ROWS:
        x = K.shape_column(shape, n)
        t = one_column(dfdb_mod, ctx, x)
        check_column(ctx, t[dfdb_mod.ALL, "x"], x)
        t.close()


@pytest.fixture(scope="module")
def sel_table(dfdb_mod, ctx):
    x, u, tt = K.selection_table()
    t = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    for name, v in (("x", x), ("u", u), ("t", tt)):
        add_raw(dfdb_mod, t, name, v)
    return t, x, K.selections(u, tt)


@pytest.mark.parametrize("name", ["none", "range", "indices", "pred10", "nothing", "empty_tiles"])
def test_selections(dfdb_mod, ctx, sel_table, name):
    t, x, sels = sel_table
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
    check_column(ctx, col, x, rows=rows)


@pytest.mark.parametrize("n", K.SHAPE_ROWS)
def test_nullable_garbage_is_neither_ranked_nor_counted(dfdb_mod, ctx, n):
    x, m = K.nullable_column(n)
    t = one_column(dfdb_mod, ctx, x, m)
    check_column(ctx, t[dfdb_mod.ALL, "x"], x, m)
    check_column(ctx, t[dfdb_mod.jr(1, 7, dfdb_mod.END), "x"], x, m, rows=np.arange(0, n, 7))
    check_column(ctx, t[dfdb_mod.jr(7, 7, dfdb_mod.END), "x"], x, m, rows=np.arange(6, n, 7))       # the missing rows alone: n = 0
    i = (np.arange(n) * 37 % 251 - 125).astype(np.int8)                                             # a narrow nullable column: garbage 127 / -128 under the flags
    i[m] = np.where(np.arange(int(m.sum())) % 2 == 0, 127, -128).astype(np.int8)
    t2 = one_column(dfdb_mod, ctx, i, m)
    check_column(ctx, t2[dfdb_mod.ALL, "x"], i, m)


def test_all_rows_missing(dfdb_mod, ctx):
    x, m = K.nullable_column(1025, all_missing=True)
    t = one_column(dfdb_mod, ctx, x, m)
    col = t[dfdb_mod.ALL, "x"]
    check_column(ctx, col, x, m)                                                                    # n = 0: counts (0, 1025, 0), any rank is BoundsError
    assert col.order_statistics([])[1] == (0, 1025, 0)
    assert col.median() is None
    with pytest.raises(ValueError):
        col.quantile(0.5)


# ---------------------------------------------------------------- the front end: median / quantile
P_CASES = (0.0, 0.5, 1.0, 1 / 3)


def same_float(a, b):
    return type(a) is type(b) and ((np.isnan(a) and np.isnan(b)) or (a == b and np.signbit(a) == np.signbit(b)))


@pytest.mark.parametrize("dtype", [np.int64, np.float64, np.float32, np.uint64, np.int8, np.bool_])
def test_median_and_quantile_values(dfdb_mod, ctx, dtype):
    for n in (1, 2, 1025, 1026):                                                                    # one value, the smallest even n, odd and even past a tile
        median_and_quantile_values(dfdb_mod, ctx, dtype, n)


def median_and_quantile_values(dfdb_mod, ctx, dtype, n):
    rng = np.random.default_rng(n)
    if dtype is np.bool_:
        x = rng.random(n) < 0.5
    elif np.dtype(dtype).kind == "f":
        x = (rng.standard_normal(n) * 100).astype(dtype)
    else:
        info = np.iinfo(dtype)
        x = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
    t = one_column(dfdb_mod, ctx, x)
    col = t[dfdb_mod.ALL, "x"]
    got, want = col.median(), K.median_ref(x)
    assert same_float(got, want), (got, want)
    assert same_float(dfdb_mod.median(col), want)
    for p in P_CASES:
        got, want = col.quantile(p), K.quantile_ref(x, p)
        assert isinstance(got, float) and same_float(got, want), (p, got, want)
    vec = dfdb_mod.quantile(col, list(P_CASES) * 3)                                                 # 12 p: 24 ranks, two calls
    assert isinstance(vec, np.ndarray) and vec.dtype == np.float64
    assert all(same_float(float(g), K.quantile_ref(x, p)) for g, p in zip(vec, list(P_CASES) * 3))
    # under a selection: every 3rd row
    rows = np.arange(0, n, 3)
    sub = t[dfdb_mod.jr(1, 3, dfdb_mod.END), "x"]
    assert same_float(sub.median(), K.median_ref(x, rows=rows)) and same_float(sub.quantile(1 / 3), K.quantile_ref(x, 1 / 3, rows=rows))


def test_median_of_extremes_does_not_overflow(dfdb_mod, ctx):
    big = np.iinfo(np.int64).max
    t = one_column(dfdb_mod, ctx, np.array([big, big], np.int64))
    assert t[dfdb_mod.ALL, "x"].median() == 9.223372036854775807e18
    t = one_column(dfdb_mod, ctx, np.array([1 << 63, 1 << 63, 0, 2**64 - 1], np.uint64))
    assert t[dfdb_mod.ALL, "x"].median() == 2.0**63 and t[dfdb_mod.ALL, "x"].quantile(1.0) == 2.0**64
    t = one_column(dfdb_mod, ctx, np.array([1.0, np.inf, -np.inf, 2.0]))
    col = t[dfdb_mod.ALL, "x"]
    assert col.median() == 1.5 and col.quantile(0.0) == -np.inf and col.quantile(1.0) == np.inf and col.quantile(0.5) == 1.5
    assert same_float(col.quantile(0.9), K.quantile_ref(np.array([1.0, np.inf, -np.inf, 2.0]), 0.9))


def test_median_and_quantile_with_missing_nan_and_empty(dfdb_mod, ctx):
    x = np.array([4.0, 1.0, 3.0, 2.0, 5.0, 9.0])
    m = np.array([0, 0, 0, 0, 0, 1], bool)
    t = one_column(dfdb_mod, ctx, x, m)
    assert t[dfdb_mod.ALL, "x"].median() is None                                                    # a missing row: missing
    with pytest.raises(ValueError, match="missing"):
        t[dfdb_mod.ALL, "x"].quantile(0.5)
    first5 = t[dfdb_mod.jr(1, 5), "x"]                                                              # the selection leaves the missing row out
    assert first5.median() == 3.0 and first5.quantile(0.25) == 2.0
    y = np.array([4.0, np.nan, 3.0, 2.0])
    t = one_column(dfdb_mod, ctx, y)
    col = t[dfdb_mod.ALL, "x"]
    assert np.isnan(col.median()) and isinstance(col.median(), np.float64)
    with pytest.raises(ValueError, match="NaN"):
        col.quantile(0.5)
    y32 = one_column(dfdb_mod, ctx, y.astype(np.float32))[dfdb_mod.ALL, "x"]
    assert np.isnan(y32.median()) and isinstance(y32.median(), np.float32)
    for c in (col, t[dfdb_mod.jr(3, 4), "x"]):
        for p in (-0.1, 1.5, [0.5, 2.0]):
            with pytest.raises(ValueError, match="probability"):
                c.quantile(p)
    empty = t[("x", lambda v: v > 100.0), "x"]                                                      # an empty selection
    with pytest.raises(ValueError, match="empty"):
        empty.median()
    with pytest.raises(ValueError, match="empty"):
        empty.quantile(0.5)


# ---------------------------------------------------------------- refusals
def test_refusals(dfdb_mod, ctx):
    from dfdb import _native as N
    x = np.arange(100, dtype=np.int64)
    t = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    add_raw(dfdb_mod, t, "x", x)
    t.add_column("s", ["a", "b"] * 50)
    with pytest.raises(ValueError, match="String"):
        t[dfdb_mod.ALL, "s"].order_statistics([1])
    with pytest.raises(ValueError, match="String"):
        t[dfdb_mod.ALL, "s"].median()
    with pytest.raises(NotImplementedError, match="materialise it as a column first"):
        (t[dfdb_mod.ALL, "x"] + 1).order_statistics([1])
    with pytest.raises(NotImplementedError, match="materialise it as a column first"):
        (t[dfdb_mod.ALL, "x"] + 1).median()
    col = t[dfdb_mod.ALL, "x"]
    for bad in (0, 101):
        with pytest.raises(IndexError):
            col.order_statistics([bad])
    q = col.view._query()
    r = np.arange(1, 18, dtype=np.int64)
    out, cnt = np.zeros(17, np.int64), np.zeros(3, np.int64)
    call = lambda k: N.load().dfdb_order_statistics(q._h, 0, r.ctypes.data, k, out.ctypes.data, None, cnt.ctypes.data)
    with pytest.raises(ValueError, match="16"):
        N.check(call(17))                                                                           # 17 ranks in one call
    with pytest.raises(ValueError):
        N.check(call(-1))
    N.check(call(16))
    assert list(out[:16]) == list(range(16)) and list(cnt) == [100, 0, 0]
    v, c = col.order_statistics(np.arange(1, 41))                                                   # the Python layer splits: 16 per call
    assert list(v) == list(range(40)) and c == (100, 0, 0)
    with pytest.raises(IndexError):
        N.check(N.load().dfdb_order_statistics(q._h, 1, r.ctypes.data, 1, out.ctypes.data, None, cnt.ctypes.data))      # no such projection column


def test_out_of_core_and_compressed_only_are_refused_by_name(dfdb_mod, ctx):
    x = (np.arange(70_001, dtype=np.int64) * 7919) % 10_007
    t = one_column(dfdb_mod, ctx, x)
    assert t[dfdb_mod.ALL, "x"].median() == K.median_ref(x)
    d = tempfile.mkdtemp(prefix="dfdb_ostat_")
    try:
        t.save(os.path.join(d, "tb"))
        ooc = dfdb_mod.open_table(os.path.join(d, "tb"), ctx=ctx, load=False)                       # opened, not loaded: out of core
        with pytest.raises(NotImplementedError, match="out of core"):
            ooc[dfdb_mod.ALL, "x"].order_statistics([1])
        with pytest.raises(NotImplementedError, match="out of core"):
            ooc[dfdb_mod.ALL, "x"].median()
        assert not ooc.resident(0)
        ooc.load()                                                                                  # loaded: answered
        assert ooc[dfdb_mod.ALL, "x"].median() == K.median_ref(x)
        ooc.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    t.compress_column("x", 2)                                                                       # what keep_compressed = 2 leaves: the LZ4 blocks alone
    assert t.resident_bytes("x")["decoded"] == 0
    with pytest.raises(NotImplementedError, match="compressed-only"):
        t[dfdb_mod.ALL, "x"].order_statistics([1])
    with pytest.raises(NotImplementedError, match="compressed-only"):
        t[dfdb_mod.ALL, "x"].quantile(0.5)
    assert dfdb_mod.nrow(t[dfdb_mod.ALL, "x"]) == len(x)                                            # (the column still answers what it answered)
