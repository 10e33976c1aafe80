"""tests/order_stat_cases.py — the numpy restatement of dfdb_order_statistics / median / quantile — pinned on hand-written answers, its columns checked to be
what their names say, and the new entry point present in every binding's symbol list.  No GPU."""
import os

import numpy as np
import pytest

import order_stat_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = np.iinfo(np.int64)


def bits(x): return K.bits_of(np.asarray(x))


def test_float_order_is_isless():
    z = K.ordered(np.array([-0.0, 0.0]))
    assert list(bits(z)) == [0x8000000000000000, 0]                   # rank 1 is -0.0, rank 2 is 0.0
    z = K.ordered(np.array([0.0, -0.0]))
    assert list(bits(z)) == [0x8000000000000000, 0]
    s = K.ordered(np.array([np.inf, np.nan, -np.inf, 1.0]))
    assert s[0] == -np.inf and s[1] == 1.0 and s[2] == np.inf and np.isnan(s[3])
    # every NaN is last and comes back canonical, whatever its sign or payload
    x = np.array([0xfff8000000000dea, 0x7ff0000000000000, 0x7ff0000000000001, 0xfff0000000000000], np.uint64).view(np.float64)
    assert list(bits(K.ordered(x))) == [0xfff0000000000000, 0x7ff0000000000000, int(K.QNAN_BITS), int(K.QNAN_BITS)]
    assert K.counts(x) == (4, 0, 2)
    # subnormals sit between the zeros and the normal numbers, on both sides
    x = np.array([1, 0x8000000000000001, 0, 0x8000000000000000, 0x0010000000000000], np.uint64).view(np.float64)
    assert list(bits(K.ordered(x))) == [0x8000000000000001, 0x8000000000000000, 0, 1, 0x0010000000000000]


def test_float32_widens_exactly():
    x = np.array([0xffc00bad, 0x00000001, 0x80000000, 0x00000000], np.uint32).view(np.float32)
    s = K.ordered(x)
    assert s.dtype == np.float64
    assert list(bits(s)) == [0x8000000000000000, 0, int(np.float64(np.float32(1e-45)).view(np.uint64)), int(K.QNAN_BITS)]


def test_integer_order():
    s = K.ordered(np.array([0, I64.max, -1, I64.min], np.int64))
    assert list(s) == [I64.min, -1, 0, I64.max]
    u = K.ordered(np.array([1 << 63, (1 << 63) - 1, 0, 2**64 - 1], np.uint64))
    assert [int(v) for v in u] == [0, (1 << 63) - 1, 1 << 63, 2**64 - 1]            # 2^63 sorts above 2^63 - 1
    assert list(K.ordered(np.array([-128, 127, 0, -1], np.int8))) == [-128, -1, 0, 127]
    assert list(K.ordered(np.array([True, False, True]))) == [0, 1, 1]
    # the image is the documented one: the sign flip of the widened value
    assert int(K.image(np.array([-1], np.int8))[0]) == 0x7fffffffffffffff and int(K.image(np.array([0], np.int32))[0]) == 1 << 63


def test_median_and_quantile_formulas():
    v = np.array([3, 1, 4, 2], np.int64)
    assert K.median_ref(v) == 2.5 and K.quantile_ref(v, 0.25) == 1.75
    assert K.median_ref(v[:3]) == 3.0 and isinstance(K.median_ref(v), np.float64)
    assert K.quantile_ref(v, 0.0) == 1.0 and K.quantile_ref(v, 1.0) == 4.0 and K.quantile_ref(v, 0.5) == 2.5 and K.quantile_ref(v, 1 / 3) == 2.0
    assert K.quantile_ref(np.array([7], np.int64), 0.3) == 7.0
    m = K.median_ref(np.array([I64.max, I64.max], np.int64))
    assert m == 9.223372036854775807e18 and np.isfinite(m)             # v/2 + v/2 in Float64: no Int64 overflow
    assert K.median_ref(np.array([1 << 63, 1 << 63], np.uint64)) == 2.0**63
    f = K.median_ref(np.array([1.0, 2.0], np.float32))
    assert isinstance(f, np.float32) and f == np.float32(1.5)
    assert np.isnan(K.median_ref(np.array([1.0, np.nan, 3.0])))
    assert K.median_ref(np.array([1.0, 2.0]), missing=[False, True]) is None
    assert K.median_ref(np.array([1.0, 2.0]), missing=[True, True]) is None         # missing wins over empty
    with pytest.raises(ValueError):
        K.median_ref(np.zeros(0))
    for bad in (dict(values=np.array([1.0, np.nan]), p=0.5), dict(values=np.zeros(0), p=0.5), dict(values=np.array([1.0]), p=1.5),
                dict(values=np.array([1.0, 2.0]), p=0.5, missing=[False, True])):
        with pytest.raises(ValueError):
            K.quantile_ref(**bad)
    # an infinite neighbour takes the other formula: (1 - g) a + g b
    assert K.quantile_ref(np.array([1.0, np.inf]), 0.5) == np.inf and K.quantile_ref(np.array([-np.inf, 1.0]), 0.0) == -np.inf


def test_selected_rows_and_missing_rows():
    v = np.array([5.0, -np.inf, 1.0, np.nan, 2.0])
    m = np.array([False, True, False, True, False])
    assert list(K.ordered(v, m)) == [1.0, 2.0, 5.0] and K.counts(v, m) == (3, 2, 0)
    assert list(K.ordered(v, m, rows=np.array([0, 1, 4]))) == [2.0, 5.0] and K.counts(v, m, rows=np.array([0, 1, 4])) == (2, 1, 0)


@pytest.mark.parametrize("n", K.SHAPE_ROWS)
def test_shape_columns_are_what_they_claim(n):
    want_dtype = {"equal": np.int64, "low_byte": np.int64, "high_byte": np.int64, "perm": np.int64, "f64_special": np.float64, "i64_extremes": np.int64,
                  "u64_mid": np.uint64, "f32": np.float32, "bool": np.bool_}
    for name in K.SHAPES:
        x = K.shape_column(name, n)
        assert len(x) == n and x.dtype == (want_dtype[name] if name in want_dtype else np.dtype(name)), name
        assert np.array_equal(K.bits_of(x), K.bits_of(K.shape_column(name, n))), name          # the same column every time it is asked for
    assert len(np.unique(K.shape_column("equal", n))) == 1
    for name, byte in (("low_byte", 0), ("high_byte", 7)):
        x = K.shape_column(name, n).view(np.uint64)
        diff = np.bitwise_or.reduce(x ^ x[0])
        assert diff == np.uint64(0xff) << np.uint64(8 * byte), (name, hex(int(diff)))          # the values differ in that byte only, in all of its bits
        assert len(np.unique(x)) > 200
    assert np.array_equal(np.sort(K.shape_column("perm", n)), np.arange(1, n + 1))
    f = K.shape_column("f64_special", n)
    fb = set(f.view(np.uint64).tolist())
    assert all(int(b) in fb for b in K.F64_SPECIAL_BITS) and len({b for b in fb if np.isnan(np.uint64(b).view(np.float64))}) >= 3
    i = K.shape_column("i64_extremes", n)
    assert I64.min in i and I64.max in i and I64.min + 1 in i and I64.max - 1 in i
    u = K.shape_column("u64_mid", n)
    assert np.uint64(1 << 63) in u and np.uint64((1 << 63) - 1) in u and np.uint64(0) in u and K.ALL1 in u
    for name in ("int8", "int16", "int32", "uint8", "uint16", "uint32"):
        x, info = K.shape_column(name, n), np.iinfo(np.dtype(name))
        assert x.min() == info.min and x.max() == info.max, name
    f32 = K.shape_column("f32", n)
    assert np.isnan(f32).any() and np.isinf(f32).any() and (f32.view(np.uint32) == 0x80000000).any()
    b = K.shape_column("bool", n)
    assert b.any() and not b.all()


def test_row_count_columns_and_selections():
    assert K.ROW_COUNTS == (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 70_001)
    for n in K.ROW_COUNTS:
        assert len(K.rowcount_column("f64", n)) == n and K.rowcount_column("i32", n).dtype == np.int32
    x, u, t = K.selection_table()
    sel = K.selections(u, t)
    n = K.N_SEL
    assert len(x) == n == 70_001 and list(sel) == ["none", "range", "indices", "pred10", "nothing", "empty_tiles"]
    assert len(sel["none"][1]) == n and len(sel["nothing"][1]) == 0 and len(sel["indices"][1]) == 777
    assert sel["range"][0] == ("range", 1, 7) and list(sel["range"][1][:3]) == [0, 7, 14]
    assert 0.08 * n < len(sel["pred10"][1]) < 0.12 * n                                          # roughly 10 %
    tiles = np.unique(sel["empty_tiles"][1] // 1024)
    assert len(sel["empty_tiles"][1]) == 3000 and len(tiles) <= 4 and n // 1024 > 60             # 3 or 4 of 69 tiles hold a row


def test_nullable_column_hides_garbage_that_would_win():
    n = 1025
    x, m = K.nullable_column(n)
    assert m.sum() == n // 7 and not m[0] and m[6]
    g = x[m]
    assert (g == -np.inf).any() and (g == np.inf).any() and np.isnan(g).any()                    # read as values they would be rank 1, rank n and a NaN
    assert np.all(g.view(np.uint64) != 0)                                                        # (nonzero bytes under every missing bit)
    s = K.ordered(x, m)
    assert np.isfinite(s).all() and K.counts(x, m) == (n - n // 7, n // 7, 0)
    x, m = K.nullable_column(n, all_missing=True)
    assert m.all() and K.counts(x, m) == (0, n, 0) and len(K.ordered(x, m)) == 0


def test_the_entry_point_is_bound_everywhere():
    import dfdb
    assert "dfdb_order_statistics" in dfdb.SYMBOLS
    for name in ("median", "quantile"):
        assert callable(getattr(dfdb, name)) and callable(getattr(dfdb.DFColumn, name))
    assert callable(dfdb.DFColumn.order_statistics)
    hdr = open(os.path.join(ROOT, "include", "dfdb.h")).read()
    assert "int32_t dfdb_order_statistics(dfdb_query* q, int32_t proj_col, const int64_t* ranks, int32_t nranks, int64_t* out_i, double* out_f, int64_t* counts);" in hdr
    for form in ("out of core", "compressed-only", "sharded"):                                   # the three refused forms are named where the contract is
        assert form in hdr, form
    jl = open(os.path.join(ROOT, "dataframedbs.jl_amd", "julia", "DataFrameDBsAMD.jl")).read()
    assert ":dfdb_order_statistics" in jl and "Statistics.median(c::DFColumn)" in jl and "Statistics.quantile(c::DFColumn, p)" in jl
