"""dfdb_sort_indices_n (csrc/sort.cpp: the most minor key sorted from the selection, every further key built from the order it finds by k_sort_rekey of
csrc/k_sort.hip and sorted by the same stable passes) against the numpy restatement of tests/sort_multi_cases.py.  Every comparison is exact: the table rows
in their order, the pairs keyed and the digit passes run and skipped summed over the keys (info), the gathered values bit for bit, and — after the calls —
dfdb_count of the same query.  Row counts lie around a 64-row bitmap word, a 1024-entry wave span of the rekey, the sort's chunk of pairs (dfdb_selftest
"sort_geometry") and 70 001: past one 65 536-row block, several workgroups, a partial last word."""
import ctypes as C
import os
import shutil
import tempfile

import numpy as np
import pytest

import order_stat_cases as K
import sort_cases as S
import sort_multi_cases as M

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 70_001)
REV2 = ((False, False), (False, True), (True, False), (True, True))


class Cols:
    """a table of raw columns (the bytes under a missing flag stay what they are) and what the restatement needs of them"""

    def __init__(self, dfdb, ctx, cols):
        from dfdb import _native as N, ir
        self.dfdb, self.names = dfdb, list(cols)
        self.values = [np.ascontiguousarray(v[0] if isinstance(v, tuple) else v) for v in cols.values()]
        self.missing = [np.ascontiguousarray(v[1], np.uint8) if isinstance(v, tuple) else None for v in cols.values()]
        self.t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
        for name, arr, m in zip(self.names, self.values, self.missing):
            N.check(N.load().dfdb_table_add_column(self.t._h, name.encode(), ir.dtype_of_numpy(arr.dtype) | (ir.NULLABLE if m is not None else 0), len(arr),
                                                   arr.ctypes.data if len(arr) else None, None, 0, m.ctypes.data if m is not None else None))

    def query(self, selector=None):
        return self.t[self.dfdb.ALL if selector is None else selector, self.dfdb.ALL]._query()

    def check(self, keys, revs, q=None, rows=None, limits=(None,), case=None):
        """the call by the columns named `keys` (major first) on query q (default: no selection; `rows`: the 0-based rows q keeps) against the restatement"""
        q = self.query() if q is None else q
        idx = [self.names.index(k) for k in keys]
        kc, km = [self.values[i] for i in idx], [self.missing[i] for i in idx]
        count0 = q.count()
        assert count0 == (len(kc[0]) if rows is None else len(rows))
        full, winfo = M.sortperm_multi_ref(kc, km, rows, revs), M.info_multi_ref(kc, km, rows)
        for limit in limits:
            got, info = q.sort_indices_n(idx, revs, limit)
            want = full if limit is None else full[:limit]
            assert got.dtype == np.int64 and np.array_equal(got, want), (case, keys, revs, limit, got[:8], want[:8])
            assert info == winfo, (case, keys, revs, limit, info, winfo)
        assert q.count() == count0                      # the selection is as it was found

    def close(self):
        self.t.close()


def chunk_pairs():
    from dfdb import _native as N
    out = (C.c_int64 * 2)()
    N.check(N.load().dfdb_selftest(b"sort_geometry", 0, out, 2))
    return int(out[0])


def three_values(n, seed=3):
    return (np.random.default_rng([n, seed]).integers(0, 3, n) - 1).astype(np.int8)


def test_row_counts(dfdb_mod, ctx):
    c = chunk_pairs()
    assert c in ROW_COUNTS                              # the counts around the sort's chunk are the ones around 4096
    for n in ROW_COUNTS:
        T = Cols(dfdb_mod, ctx, {"g": three_values(n), "f": K.rowcount_column("f64", n), "i": K.rowcount_column("i32", n)})
        for revs in REV2:
            T.check(["g", "f"], revs, case=n)
        T.check(["g", "i"], (True, False), case=n)
        T.check(["g", "g", "i"], (False, True, True), case=n)
        T.close()


# ---------------------------------------------------------------- every dtype of the kernels' dispatch list, ~40 distinct values each so that both keys decide
def dtype_columns(n):
    rng = np.random.default_rng([n, 11])
    cols = {}
    for name in ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"):
        i = np.iinfo(name)
        pool = np.concatenate([np.array([i.min, i.min + 1, i.max - 1, i.max], name), rng.integers(i.min, i.max, 36, dtype=name, endpoint=True)])
        cols[name] = rng.choice(pool, n)
    cols["bool"] = rng.random(n) < 0.4
    f64 = np.concatenate([K.F64_SPECIAL_BITS, rng.standard_normal(27).view(np.uint64)])
    cols["float64"] = rng.choice(f64, n).view(np.float64)
    f32 = np.concatenate([K.F32_SPECIAL_BITS, rng.standard_normal(31).astype(np.float32).view(np.uint32)])
    cols["float32"] = rng.choice(f32, n).view(np.float32)
    cols["g"] = three_values(n)
    cols["perm"] = (rng.permutation(n) + 1).astype(np.int64)
    return cols


def test_every_dtype_as_major_and_as_minor_key(dfdb_mod, ctx):
    n = 4097
    cols = dtype_columns(n)
    T = Cols(dfdb_mod, ctx, cols)
    q = T.query()
    for name in cols:
        if name in ("g", "perm"):
            continue
        for revs in ((False, False), (True, True)) if name not in ("float32", "float64") else REV2:
            T.check([name, "perm"], revs, q=q, case=name)         # major: its ties (every NaN one value, -0.0 below 0.0) are broken by the minor key
            T.check(["g", name], revs, q=q, case=name)            # minor: it orders the rows within the three values of the major key
    T.close()


def test_what_the_major_key_leaves_to_the_minor_one(dfdb_mod, ctx):
    n = 70_001
    minor = K.rowcount_column("i32", n)
    T = Cols(dfdb_mod, ctx, {"three": three_values(n), "distinct": K.shape_column("perm", n), "equal": K.shape_column("equal", n), "m": minor})
    q = T.query()
    for major in ("three", "distinct", "equal"):
        for revs in REV2:
            T.check([major, "m"], revs, q=q, case=major)
    # an all-equal major key takes no pass: the rekey alone, and the order the minor key left comes through it untouched
    single = q.sort_indices(T.names.index("m"))
    both, info = q.sort_indices_n([T.names.index("equal"), T.names.index("m")])
    assert np.array_equal(both, single[0]) and info == (n, 2 * n, single[1][2], single[1][3] + 8)
    T.close()


def nullable_columns(n):
    x, m = K.nullable_column(n)                                     # Float64: -Inf / NaN / Inf under the flags
    b = (np.arange(n) * 37 % 251 - 125).astype(np.int8)             # Int8: 127 / -128 under other flags
    bm = np.arange(n) % 5 == 3
    b[bm] = np.where(np.arange(int(bm.sum())) % 2 == 0, 127, -128).astype(np.int8)
    g = three_values(n)
    gm = np.arange(n) % 11 == 0
    g[gm] = 127
    y, am = K.nullable_column(n, all_missing=True)
    return {"x": (x, m), "b": (b, bm), "g": (g, gm), "none": (y, am), "plain": K.rowcount_column("i32", n)}


def test_nullable_garbage_never_moves_a_row(dfdb_mod, ctx):
    for n in (1025, 70_001):
        T = Cols(dfdb_mod, ctx, nullable_columns(n))
        q = T.query()
        for revs in REV2:
            T.check(["g", "plain"], revs, q=q, case=n)              # missing in the major key only
            T.check(["plain", "x"], revs, q=q, case=n)              # in the minor key only (the major key has nearly no ties) ...
            T.check(["b", "x"], revs, q=q, case=n)                  # ... and under a major key with ties
            T.check(["g", "b"], revs, q=q, case=n)                  # in both, in different rows and (every 55th row) in the same
            T.check(["none", "b"], revs, q=q, case=n)               # in all rows of the major key
            T.check(["g", "none"], revs, q=q, case=n)               # in all rows of the minor key
        T.check(["none", "none"], (False, True), q=q, case=n)
        q7 = T.query(dfdb_mod.jr(7, 7, dfdb_mod.END))               # the rows missing in x alone
        T.check(["x", "b"], (False, True), q=q7, rows=np.arange(6, n, 7), limits=(None, 3), case=n)
        T.close()


def test_three_keys_eight_keys_and_a_column_twice(dfdb_mod, ctx):
    n = 8193
    rng = np.random.default_rng(8193)
    cols = {f"k{j}": rng.integers(0, 2, n).astype(np.int8) for j in range(8)}
    cols.update({"f": K.rowcount_column("f64", n), "u": rng.integers(0, 50, n).astype(np.uint16)})
    T = Cols(dfdb_mod, ctx, cols)
    q = T.query()
    T.check(["k0", "u", "f"], (True, False, True), q=q)
    T.check(["u", "k1", "k2"], (False, True, False), q=q)
    eight = [f"k{j}" for j in range(8)]
    T.check(eight, (False, True, False, False, True, True, False, True), q=q)
    T.check(eight[:7] + ["f"], (True,) * 8, q=q)
    T.check(["u", "u"], (False, False), q=q)
    T.check(["u", "u"], (False, True), q=q)                          # the major direction decides; the minor copy never sees two different values
    T.check(["u", "f", "u"], (True, False, False), q=q)
    T.close()


def test_selections(dfdb_mod, ctx):
    x, u, tt = K.selection_table()
    T = Cols(dfdb_mod, ctx, {"x": x, "u": u, "t": tt, "g": three_values(len(x))})
    sels = dict(K.selections(u, tt))
    sels["pred90"] = (("pred", "u", "<", 90), np.flatnonzero(u < 90))
    for name in ("none", "range", "indices", "pred10", "pred90", "nothing", "empty_tiles"):
        spec, rows = sels[name]
        if spec is None:
            sel = None
        elif spec[0] == "range":
            sel = dfdb_mod.jr(spec[1], spec[2], dfdb_mod.END)
        elif spec[0] == "indices":
            sel = list(spec[1])
        else:
            k = spec[3]
            sel = (spec[1], (lambda c: c < k) if spec[2] == "<" else (lambda c: c == k))
        q = T.query(sel)
        T.check(["g", "x"], (False, True), q=q, rows=rows, limits=(None, 10), case=name)
        T.check(["u", "g", "x"], (True, False, False), q=q, rows=rows, case=name)
    T.close()


def test_limit_is_the_prefix(dfdb_mod, ctx):
    n = 3 * chunk_pairs() + 17
    cols = nullable_columns(n)
    T = Cols(dfdb_mod, ctx, cols)
    q = T.query()
    limits = (0, 1, 64, n - 1, n, n + 5)
    T.check(["g", "x"], (False, True), q=q, limits=limits)
    T.check(["b", "plain"], (True, False), q=q, limits=limits)
    rows = np.arange(2, n, 3)
    q3 = T.query(dfdb_mod.jr(3, 3, dfdb_mod.END))
    T.check(["g", "x"], (True, True), q=q3, rows=rows, limits=(0, 1, 64, len(rows) - 1, len(rows), len(rows) + 5))
    T.close()


def test_one_key_is_sort_indices(dfdb_mod, ctx):
    n = chunk_pairs() + 1
    T = Cols(dfdb_mod, ctx, nullable_columns(n))
    q = T.query(dfdb_mod.jr(1, 2, dfdb_mod.END))
    for name in ("x", "b", "plain", "none"):
        i = T.names.index(name)
        for rev in (False, True):
            for limit in (None, 0, 1, 10, n // 2, n):
                a, ia = q.sort_indices(i, rev, limit)
                b, ib = q.sort_indices_n([i], [rev], limit)
                assert np.array_equal(a, b) and ia == ib, (name, rev, limit, ia, ib)
    T.close()


def test_device_output_feeds_gather_rows_and_sort_view_takes_a_list(dfdb_mod, ctx):
    import torch
    n = chunk_pairs() + 1
    rng = np.random.default_rng(n)
    cols = {"g": three_values(n), "i": rng.integers(-50, 50, n).astype(np.int32), "d": rng.standard_normal(n).round(2) + 0.0}
    T = Cols(dfdb_mod, ctx, cols)
    v = T.t[dfdb_mod.ALL, dfdb_mod.ALL]
    q = v._query()
    want = M.sortperm_multi_ref([cols["g"], cols["i"]], [None, None], None, [True, False])
    buf = torch.full((n + 2,), -7, dtype=torch.int64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()                # (the fill runs on torch's stream, the sort on the engine's own: order them)
    none, info = q.sort_indices_n([0, 1], [True, False], None, dev_ptr=buf.data_ptr() + 8, cap=n)
    ctx.synchronize()
    h = buf.cpu().numpy()
    assert none is None and info[0] == n and h[0] == -7 and h[-1] == -7 and np.array_equal(h[1:-1], want)
    got = q.gather_rows(dev_ptr=buf.data_ptr() + 8, n=n)                                            # the rows never leave the device
    for name, g in zip(T.names, got):
        assert np.array_equal(K.bits_of(g), K.bits_of(cols[name][want - 1])), name
    buf.fill_(-7)
    torch.cuda.synchronize()
    q.sort_indices_n([0, 1], [True, False], None, dev_ptr=buf.data_ptr(), cap=5)                    # a capacity below the count: nothing beyond it is written
    ctx.synchronize()
    h = buf.cpu().numpy()
    assert np.array_equal(h[:5], want[:5]) and np.all(h[5:] == -7)
    assert np.array_equal(dfdb_mod.sortperm_by(v, ["g", "i"], rev=[True, False]), want)
    assert np.array_equal(dfdb_mod.sortperm_by(v, ["g", "i"], rev=[True, False], limit=9), want[:9])
    assert np.array_equal(dfdb_mod.sortperm_by(v, "d", rev=True), S.sortperm_ref(cols["d"], rev=True))
    # sort!(materialize(v), by; rev): no missing, no NaN, no -0.0 — there pandas' stable order is the same
    sub = T.t[("i", lambda c: c < 30), dfdb_mod.ALL]
    keep = np.flatnonzero(cols["i"] < 30)
    try:
        import pandas as pd
    except ImportError:
        pd = None
    for by, rev in ((["g", "i"], [False, True]), (["i", "d", "g"], [True, True, False]), (["g", "d"], False)):
        df = dfdb_mod.sort_view(sub, by, rev=rev, limit=None)
        revs = [rev] * len(by) if isinstance(rev, bool) else rev
        if pd is not None:
            ref = pd.DataFrame({k: cols[k][keep] for k in T.names}).sort_values(by, ascending=[not r for r in revs], kind="stable")
            want_cols = {k: ref[k].to_numpy() for k in T.names}
        else:
            w = M.sortperm_multi_ref([cols[k] for k in by], [None] * len(by), keep, revs)
            want_cols = {k: cols[k][w - 1] for k in T.names}
        assert list(df.columns) == T.names and len(df) == len(keep)
        for k in T.names:
            assert np.array_equal(K.bits_of(df[k].to_numpy()), K.bits_of(want_cols[k])), (by, rev, k)
    df = dfdb_mod.sort_view(sub, ["g", "i"], rev=[False, True], limit=100)
    w = M.sortperm_multi_ref([cols["g"], cols["i"]], [None, None], keep, [False, True], 100)
    assert len(df) == 100 and np.array_equal(df["d"].to_numpy(), cols["d"][w - 1])
    with pytest.raises(ValueError):
        dfdb_mod.sort_view(sub, ["g", "i"], rev=[False])
    T.close()


def test_refusals_name_the_form(dfdb_mod, ctx):
    from dfdb import _native as N
    x = (np.arange(70_001, dtype=np.int64) * 7919) % 10_007
    T = Cols(dfdb_mod, ctx, {"x": x, "g": three_values(len(x))})
    t = T.t
    t.add_column("s", ["a", "b", "c"] * 23_333 + ["a", "b"])
    q = t[dfdb_mod.ALL, dfdb_mod.ALL]._query()                      # x, g, s
    want = M.sortperm_multi_ref([T.values[1], x], [None, None])
    for keys in ([2, 0], [0, 2], [1, 0, 2]):                         # a String key in a major and in a minor position
        with pytest.raises(NotImplementedError, match="sorting by a String column"):
            q.sort_indices_n(keys)
    cv = dfdb_mod.view_from_columns(a=t[dfdb_mod.ALL, "x"], b=t[dfdb_mod.ALL, "x"] + 1)._query()
    for keys in ([1, 0], [0, 1]):
        with pytest.raises(NotImplementedError, match="sorting by a computed column"):
            cv.sort_indices_n(keys)
    for bad in ([0, 3], [-1, 0], [3, 0]):
        with pytest.raises(IndexError):
            q.sort_indices_n(bad)
    L = N.load()
    two, one = (C.c_int32 * 9)(*([0, 1] + [0] * 7)), (C.c_int32 * 9)()
    for nkeys in (0, 9, -1):
        with pytest.raises(ValueError, match="sort keys"):
            N.check(L.dfdb_sort_indices_n(q._h, two, one, nkeys, -1, None, 0, N.MEM_HOST, None, None))
    with pytest.raises(ValueError):
        N.check(L.dfdb_sort_indices_n(q._h, None, one, 2, -1, None, 0, N.MEM_HOST, None, None))
    with pytest.raises(ValueError):
        N.check(L.dfdb_sort_indices_n(q._h, two, None, 2, -1, None, 0, N.MEM_HOST, None, None))
    for flags in ((2, 0), (0, 2), (1, 3)):
        with pytest.raises(ValueError, match="sort flags"):
            N.check(L.dfdb_sort_indices_n(q._h, two, (C.c_int32 * 2)(*flags), 2, -1, None, 0, N.MEM_HOST, None, None))
    assert np.array_equal(q.sort_indices_n([1, 0])[0], want)         # the refusals left the query as it was
    d = tempfile.mkdtemp(prefix="dfdb_sortn_")
    try:
        T2 = Cols(dfdb_mod, ctx, {"x": x, "g": T.values[1]})
        T2.t.save(os.path.join(d, "tb"))
        ooc = dfdb_mod.open_table(os.path.join(d, "tb"), ctx=ctx, load=False)                       # opened, not loaded: out of core
        with pytest.raises(NotImplementedError, match="out of core"):
            ooc[dfdb_mod.ALL, dfdb_mod.ALL]._query().sort_indices_n([1, 0])
        ooc.load()                                                                                  # loaded: answered
        assert np.array_equal(ooc[dfdb_mod.ALL, dfdb_mod.ALL]._query().sort_indices_n([1, 0])[0], want)
        ooc.close()
        T2.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    t.compress_column("x", 2)                                                                       # what keep_compressed = 2 leaves: the LZ4 blocks alone
    assert t.resident_bytes("x")["decoded"] == 0
    for keys in ([0, 1], [1, 0]):
        with pytest.raises(NotImplementedError, match="compressed-only"):
            t[dfdb_mod.ALL, ["x", "g"]]._query().sort_indices_n(keys)
    assert dfdb_mod.nrow(t[dfdb_mod.ALL, "x"]) == len(x)                                            # (the column still answers what it answered)
    T.close()
