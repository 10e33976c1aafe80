"""The edge values of csrc/value_rules.hpp (tests/test_value_rules_cpu.py pins its host side) carried through every device form that uses the rules, so that a
copy that was missed or mis-replaced fails on the device too.  groupreduce, by unique.cpp's thresholds (the profile notes say which form ran):
  7 groups      an 8-byte value column through k_group_acc_hash_lds (group_accumulate.hash_lds), a narrow one through the 1024-group k_group_acc;
  2 000 groups  a dense key: an 8-byte value through k_group_acc_dense_lds (group_accumulate.dense_lds), a narrow one through the 9216-group k_group_acc;
  9 300 groups  above kGroupsInLds = 9216: by radix (group_radix.taken), and with ctx option unique_radix = 0 through the global atomics of k_group_acc<0>,
                whose hot slots the one key that holds 30 % of the rows fills.  The radix form's own hot slots are compiled in only for a column whose
                sample shows more than 65 536 rows in one partition (unique.cpp RadixRun::skewed): a second table of 230 000 rows, group_radix.skewed.
Then the whole-column aggregates through k_reduce_* and through the scan-fused aggregate, and unique by the hash table and by radix (unique.cpp unique_radix:
4 << 20 selected rows and 131072 distinct values at least).  The expectations are numpy restatements of Julia's rules: any NaN gives NaN; among equal zeros
the minimum is -0.0 if one is present and the maximum 0.0; isequal keys (one NaN, the two zeros apart).  Float64 sums: |err| <= 64 eps sum|x|."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS = 40_037
QNAN = np.uint64(0x7ff8000000000000)


def f64_from_bits(bits): return np.array(bits, np.uint64).view(np.float64)


def canon(x):
    """Float64 values as bit patterns with every NaN folded onto one"""
    u = np.ascontiguousarray(x, np.float64).view(np.uint64).copy()
    u[np.isnan(x)] = QNAN
    return u


def order_key(x):
    """a uint64 per finite-or-infinite Float64 that sorts as Julia's isless does on them: -0.0 below 0.0"""
    u = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def order_key_inv(k):
    return np.where(k >> np.uint64(63) != 0, k & np.uint64((1 << 63) - 1), ~k).view(np.float64)


def julia_minmax(v, starts, stat):
    """per segment of v (float64, sorted by group): Base.minimum / Base.maximum"""
    nan = np.isnan(v)
    k = order_key(np.where(nan, 0.0, v))
    red = (np.minimum if stat == "min" else np.maximum).reduceat(k, starts)
    out = order_key_inv(red).copy()
    out[np.add.reduceat(nan.astype(np.int64), starts) > 0] = np.nan
    return out


@pytest.fixture(scope="module")
def table(dfdb_mod, ctx):
    rng = np.random.default_rng(20261018)
    n = N_ROWS
    i7 = rng.integers(0, 7, n)
    k7 = i7.astype(np.int64) * 10**15 - 5                                                       # (too wide a span for the dense form)
    i2000 = rng.integers(0, 2000, n)
    k2000 = i2000.astype(np.int64) * 7 - 40_000                                                 # (a span of 14 000: the dense table fits k_group_acc_dense_lds's LDS)
    i9300 = np.concatenate([np.arange(9300), np.where(rng.random(n - 9300) < 0.3, 0, rng.integers(0, 9300, n - 9300))])      # every key is there; key 0 holds 30 % of the rows
    rng.shuffle(i9300)
    k9300 = i9300.astype(np.int64) * 40_503 - 3_000_000_000
    g2 = i2000 % 5
    x = rng.integers(-3, 4, n).astype(np.float64) / 2.0
    x[(x == 0) & (rng.random(n) < 0.5)] = -0.0
    x[g2 == 0] = np.abs(x[g2 == 0]); x[(g2 == 0) & (x == 0) & (rng.random(n) < 0.5)] = -0.0      # zeros and positives: the minimum is a zero
    x[g2 == 1] = -np.abs(x[g2 == 1]); x[(g2 == 1) & (x == 0) & (rng.random(n) < 0.5)] = 0.0      # zeros and negatives: the maximum is a zero
    rare = (g2 == 2) & (i7 < 2) & (i9300 % 3 == 0)                                               # (the hot key among them)
    xb = x.view(np.uint64)
    xb[rare & (rng.random(n) < 0.3)] = np.uint64(0x7ff8000000000001)                            # NaN, two payloads and both signs
    xb[rare & (rng.random(n) < 0.3)] = np.uint64(0xfff8000000000dea)
    x[(g2 == 3) & (rng.random(n) < 0.05)] = np.inf
    x[(g2 == 4) & (rng.random(n) < 0.05)] = -np.inf
    x32 = x.astype(np.float32)
    x32.view(np.uint32)[np.isnan(x) & (rng.random(n) < 0.5)] = np.uint32(0xffc00bad)
    z = np.abs(rng.integers(0, 4, n).astype(np.float64)); z[(z == 0) & (rng.random(n) < 0.5)] = -0.0      # no NaN: whole-column minimum -0.0, maximum of -z is 0.0
    cols = {"k7": k7, "k2000": k2000, "k9300": k9300, "x": x, "x32": x32, "z": z, "nz": -z}
    for t in (np.int8, np.int16, np.int32, np.uint8, np.uint16, np.uint32):
        i = np.iinfo(t)
        v = rng.integers(i.min, int(i.max) + 1, n).astype(t)
        v[rng.random(n) < 0.02] = i.min; v[rng.random(n) < 0.02] = i.max
        cols[np.dtype(t).name] = v
    tb = dfdb_mod.DFTable.from_columns(cols, block_size=65536, ctx=ctx)
    yield tb, cols
    tb.close()


def grouped(keys):
    """rows sorted by group in order of first appearance: (row order, segment starts, counts)"""
    uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), np.int64); rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))
    gid = rank[inv]
    order = np.argsort(gid, kind="stable")
    cnt = np.bincount(gid, minlength=len(uniq))
    return order, np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt, keys[np.sort(first)]


VALUE_COLS = ["x", "x32", "int8", "int16", "int32", "uint8", "uint16", "uint32"]


@pytest.mark.parametrize("by,radix,want_taken", [("k7", 1, 0), ("k2000", 1, 0), ("k9300", 1, 1), ("k9300", 0, 0)])
def test_groupreduce_carries_the_edge_values_through_every_accumulate_form(dfdb_mod, ctx, table, by, radix, want_taken):
    tb, cols = table
    order, starts, cnt, first_keys = grouped(cols[by])
    for col in VALUE_COLS:
        v = cols[col][order]
        for stat in ("min", "max", "sum"):
            ctx.set_option("unique_radix", radix); ctx.profile(True)
            try:
                df = dfdb_mod.groupreduce(tb, by, col, stat)
                note = {k: ctx.profile_get(k)[0] for k in ("group_radix.taken", "group_radix.skewed", "group_accumulate.hash_lds", "group_accumulate.dense_lds")}
            finally:
                ctx.profile(False); ctx.set_option("unique_radix", 1)
            wide = cols[col].dtype.itemsize == 8
            want_note = {"group_radix.taken": want_taken, "group_radix.skewed": 0,      # (skewed takes 65 536 rows of one partition: the test below)
                         "group_accumulate.hash_lds": int(by == "k7" and wide), "group_accumulate.dense_lds": int(by == "k2000" and wide)}
            assert note == want_note, (by, col, stat, note)                                     # (none of the four: the 1024- / 9216-group or the global k_group_acc)
            assert np.array_equal(df[by].to_numpy(), first_keys) and np.array_equal(df["count"].to_numpy(), cnt), (by, col, stat)
            got = df[stat].to_numpy()
            if v.dtype.kind == "f":
                v64 = v.astype(np.float64)
                if stat == "sum":
                    with np.errstate(invalid="ignore"):
                        want = np.add.reduceat(v64, starts)
                        absum = np.add.reduceat(np.abs(np.where(np.isfinite(v64), v64, 0.0)), starts)
                    fin = np.isfinite(want)
                    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(canon(got[~fin]), canon(want[~fin])), (by, col)
                    assert np.all(np.abs(got[fin] - want[fin]) <= 64 * np.finfo(np.float64).eps * absum[fin]), (by, col)
                else:
                    want = julia_minmax(v64, starts, stat)
                    assert np.array_equal(canon(got), canon(want)), (by, col, stat, np.flatnonzero(canon(got) != canon(want))[:5])
            else:
                v64 = v.astype(np.int64)
                want = (np.add if stat == "sum" else (np.minimum if stat == "min" else np.maximum)).reduceat(v64, starts)
                assert np.array_equal(np.asarray(got).astype(np.int64), want), (by, col, stat)


def test_groupreduce_by_radix_reduces_a_hot_keys_edge_values_in_the_partition_pass(dfdb_mod, ctx):
    """the HOT forms of k_radix_partition: one key holds 35 % of 230 000 rows (more than the 65 536 the sample asks for), NaN, both zeros and the infinities among
    its values and among the others'"""
    rng = np.random.default_rng(7)
    n = 230_000
    ik = np.concatenate([np.arange(9300), np.where(rng.random(n - 9300) < 0.35, 17, rng.integers(0, 9300, n - 9300))])
    rng.shuffle(ik)
    k = ik.astype(np.int64) * 40_503 - 3_000_000_000
    x = rng.integers(-3, 4, n).astype(np.float64) / 2.0
    x[(x == 0) & (rng.random(n) < 0.5)] = -0.0
    x[ik % 4 == 0] = np.abs(x[ik % 4 == 0]); x[ik % 4 == 2] = -np.abs(x[ik % 4 == 2])             # groups whose minimum / maximum is a zero of either sign
    x.view(np.uint64)[(ik % 4 == 3) & (rng.random(n) < 0.2)] = np.uint64(0xfff8000000000dea)
    x[(ik % 8 == 1) & (rng.random(n) < 0.1)] = np.inf                                             # (17 is 1 mod 8: the hot key holds zeros, infinities and finite values)
    x32 = x.astype(np.float32)
    u8 = rng.integers(0, 256, n).astype(np.uint8); u8[rng.random(n) < 0.02] = 255; u8[rng.random(n) < 0.02] = 0
    cols = {"k": k, "x": x, "x32": x32, "uint8": u8}
    order, starts, cnt, first_keys = grouped(k)
    tb = dfdb_mod.DFTable.from_columns(cols, block_size=65536, ctx=ctx)
    try:
        for col in ("x", "x32", "uint8"):
            v64 = cols[col][order].astype(np.float64 if cols[col].dtype.kind == "f" else np.int64)
            for stat in ("min", "max", "sum"):
                ctx.profile(True)
                try:
                    df = dfdb_mod.groupreduce(tb, "k", col, stat)
                    note = [ctx.profile_get(key)[0] for key in ("group_radix.taken", "group_radix.skewed")]
                finally:
                    ctx.profile(False)
                assert note == [1, 1], (col, stat, note)
                assert np.array_equal(df["k"].to_numpy(), first_keys) and np.array_equal(df["count"].to_numpy(), cnt), (col, stat)
                got = df[stat].to_numpy()
                if v64.dtype.kind != "f":
                    want = (np.add if stat == "sum" else (np.minimum if stat == "min" else np.maximum)).reduceat(v64, starts)
                    assert np.array_equal(np.asarray(got).astype(np.int64), want), (col, stat)
                elif stat == "sum":
                    with np.errstate(invalid="ignore"):
                        want = np.add.reduceat(v64, starts)
                        absum = np.add.reduceat(np.abs(np.where(np.isfinite(v64), v64, 0.0)), starts)
                    fin = np.isfinite(want)
                    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(canon(got[~fin]), canon(want[~fin])), col
                    assert np.all(np.abs(got[fin] - want[fin]) <= 64 * np.finfo(np.float64).eps * absum[fin]), col
                else:
                    assert np.array_equal(canon(got), canon(julia_minmax(v64, starts, stat))), (col, stat)
    finally:
        tb.close()


def test_whole_column_minimum_and_maximum_agree_between_the_reduce_kernels_and_the_scan(dfdb_mod, ctx, table):
    tb, cols = table
    bits = lambda d: struct.unpack("<Q", struct.pack("<d", d))[0]
    views = {                                                                                  # (a fresh view per aggregate: the hint acts on a query's FIRST execution)
        "reduce": lambda col: tb,
        "reduce under a predicate": lambda col: tb[("k7", lambda c: c > -1_000_000), dfdb_mod.ALL],
        "scan": lambda col: tb[(col, lambda c: c != 1e300), dfdb_mod.ALL],                     # on the aggregated column itself, true for a NaN too: the scan reduces what it holds
    }
    for col, want_min, want_max in (("x", float("nan"), float("nan")), ("z", -0.0, 3.0), ("nz", -3.0, 0.0)):
        for how, make in views.items():
            for stat, want in (("min", want_min), ("max", want_max)):
                view = make(col)
                ctx.profile(True)
                try:
                    got = getattr(view[dfdb_mod.ALL, col], stat)()
                    partials = ctx.profile_get("reduce_partials")[0]                            # launches of the reduction over the scan's per-tile partials
                finally:
                    ctx.profile(False)
                assert (partials > 0) == (how == "scan"), (col, how, stat, partials)
                assert (got != got and want != want) or bits(got) == bits(want), (col, how, stat, got, want)
                assert dfdb_mod.nrow(view) == N_ROWS                                            # every row was kept


def unique_images(x):
    img = canon(x) if x.dtype == np.float64 else np.where(np.isnan(x), np.uint32(0x7fc00000), x.view(np.uint32))
    _, first = np.unique(img, return_index=True)
    return img[np.sort(first)]


def check_unique(got, x):
    want = unique_images(x)
    gi = canon(got) if x.dtype == np.float64 else np.where(np.isnan(got), np.uint32(0x7fc00000), np.ascontiguousarray(got, np.float32).view(np.uint32))
    assert np.array_equal(gi, want)
    assert np.isnan(got).sum() == 1 and (np.signbit(got) & (got == 0)).sum() == 1 and ((~np.signbit(got)) & (got == 0)).sum() == 1      # one NaN, both zeros


def test_unique_over_float_keys_keeps_one_nan_and_both_zeros(dfdb_mod, ctx, table):
    tb, cols = table
    ctx.set_option("unique_radix", 0)
    try:
        for col in ("x", "x32"):
            check_unique(np.asarray(tb[dfdb_mod.ALL, col].unique()), cols[col])
    finally:
        ctx.set_option("unique_radix", 1)


def test_unique_by_radix_keeps_one_nan_and_both_zeros(dfdb_mod, ctx):
    n = 4 << 20                                                                                # unique.cpp unique_radix: the smallest selection it takes
    x = np.arange(n, dtype=np.float64) - 1000.0                                                # distinct finite values (0.0 among them)
    x.view(np.uint64)[[5, 3_000_000]] = [0x7ff8000000000001, 0xfff8000000000dea]
    x[[7, 2_000_000]] = -0.0
    x[[11, 12]] = [np.inf, -np.inf]
    x32 = x.astype(np.float32)                                                                 # (integers below 2^24: still distinct)
    x32.view(np.uint32)[3_000_000] = 0xffc00bad
    tb = dfdb_mod.DFTable.from_columns({"x": x, "x32": x32}, block_size=65536, ctx=ctx)
    try:
        for col, v in (("x", x), ("x32", x32)):
            ctx.profile(True)
            try:
                got = np.asarray(tb[dfdb_mod.ALL, col].unique())
                taken = ctx.profile_get("unique_radix.taken")[0]
            finally:
                ctx.profile(False)
            assert taken == 1, col
            check_unique(got, v)
    finally:
        tb.close()
