"""dfdb_query_join / dfdb_query_join_fetch (csrc/join.cpp over csrc/k_join.hip: the right side's sorted pairs, one probe launch, one scan, one expand launch)
against the brute-force restatement of tests/join_cases.py.  Every comparison is exact: both row lists, the number of pairs, info[0:4] — and, after the calls,
dfdb_count and dfdb_select_indices of both queries.  The sizes are the smallest at which each piece can go wrong: row counts around a wave's round of 64, a
1024-entry group, the sort's chunk of pairs and several workgroups; right sides around every power of two the search steps through."""
import ctypes as C

import numpy as np
import pytest

import join_cases as J
import order_stat_cases as K

pytestmark = pytest.mark.gpu
SENTINEL = -7


def add_raw(dfdb, t, name, values, missing=None):
    """a column exactly as given: the bytes under a missing flag stay what they are"""
    from dfdb import _native as N, ir
    arr = np.ascontiguousarray(values)
    dt = ir.dtype_of_numpy(arr.dtype)
    m = None if missing is None else np.ascontiguousarray(missing, np.uint8)
    N.check(N.load().dfdb_table_add_column(t._h, name.encode(), dt | (ir.NULLABLE if m is not None else 0), len(arr), arr.ctypes.data if len(arr) else None, None, 0,
                                           m.ctypes.data if m is not None else None))


def one_column(dfdb, ctx, values, missing=None, name="x"):
    t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    add_raw(dfdb, t, name, values, missing)
    return t


def chunk_pairs():
    from dfdb import _native as N
    out = (C.c_int64 * 2)()
    N.check(N.load().dfdb_selftest(b"sort_geometry", 0, out, 2))
    return int(out[0])


def check_join(lcol, lvals, rcol, rvals, lmiss=None, rmiss=None, lrows=None, rrows=None, lbase=0, rbase=0, kinds=J.KINDS, case=None):
    """lcol / rcol: the DFColumns of the two keys under selections that keep the 0-based lrows / rrows (None: all)"""
    ql, qr = lcol.view._query(), rcol.view._query()
    before = (ql.count(), ql.indices().copy(), qr.count(), qr.indices().copy())
    want = J.join_ref_all(lvals, lmiss, lrows, rvals, rmiss, rrows, lbase, rbase, kinds)
    for kind in kinds:
        wl, wr, winfo = want[kind]
        n, info = ql.join_count(qr, 0, 0, J.KIND_CODE[kind])
        assert n == len(wl) and info[:4] == winfo, (case, kind, n, len(wl), info, winfo)
        gl, gr = ql.join_fetch(n)
        assert gl.dtype == np.int64 and np.array_equal(gl, wl), (case, kind, gl[:8], wl[:8])
        assert np.array_equal(gr, wr), (case, kind, gr[:8], wr[:8])
    assert (ql.count(), qr.count()) == (before[0], before[2]) and np.array_equal(ql.indices(), before[1]) and np.array_equal(qr.indices(), before[3]), case


def test_left_row_counts(dfdb_mod, ctx):
    right = J.unique_keys(1025)
    tr = one_column(dfdb_mod, ctx, right)
    for nl in J.LEFT_COUNTS:
        left = J.probe_keys(nl, right)
        tl = one_column(dfdb_mod, ctx, left)
        check_join(tl[dfdb_mod.ALL, "x"], left, tr[dfdb_mod.ALL, "x"], right, case=nl)
        tl.close()
    tr.close()


def test_right_row_counts(dfdb_mod, ctx):
    c = chunk_pairs()
    for nr in J.RIGHT_COUNTS_FIXED + (c - 1, c, c + 1):
        right = J.unique_keys(nr)
        left = J.probe_keys(1025, right)
        tl, tr = one_column(dfdb_mod, ctx, left), one_column(dfdb_mod, ctx, right)
        check_join(tl[dfdb_mod.ALL, "x"], left, tr[dfdb_mod.ALL, "x"], right, case=nr)
        tl.close()
        tr.close()


def test_edge_keys_of_every_dtype(dfdb_mod, ctx):
    for dt in J.EDGE_DTYPES:
        left, right = J.edge_sides(dt, 300, 200)
        tl, tr = one_column(dfdb_mod, ctx, left), one_column(dfdb_mod, ctx, right)
        check_join(tl[dfdb_mod.ALL, "x"], left, tr[dfdb_mod.ALL, "x"], right, case=np.dtype(dt).name)
        tl.close()
        tr.close()


def multiplicity_shapes():
    """name -> (left keys, right keys)"""
    ramp_l = np.concatenate([np.arange(64), np.full(100, 99)]).astype(np.int64)          # the first round's lanes emit 0, 1, 2, .. 63 pairs
    ramp_r = np.repeat(np.arange(64), np.arange(64)).astype(np.int64)
    gaps_l = np.concatenate([np.full(1024, 5), np.full(2048, -1), np.full(1000, 6), np.full(1024, -2), np.full(10, 5)]).astype(np.int64)   # groups 1, 2 and 4 emit nothing
    gaps_r = np.array([6, 5, 5, 7], np.int64)
    return {"one_against_5000": (np.array([3], np.int64), np.full(5000, 3, np.int64)),
            "1024_against_70": (np.full(1024, 8, np.int64), np.full(70, 8, np.int64)),
            "300x300": (np.full(300, 1, np.int64), np.full(300, 1, np.int64)),
            "ramp": (ramp_l, ramp_r), "empty_groups": (gaps_l, gaps_r)}


def test_multiplicity(dfdb_mod, ctx):
    for name, (left, right) in multiplicity_shapes().items():
        tl, tr = one_column(dfdb_mod, ctx, left), one_column(dfdb_mod, ctx, right)
        check_join(tl[dfdb_mod.ALL, "x"], left, tr[dfdb_mod.ALL, "x"], right, case=name)
        tl.close()
        tr.close()


def test_missing_keys_match_nothing(dfdb_mod, ctx):
    (lx, lm), (rx, rm) = J.nullable_side(4097, 3), J.nullable_side(3001, 4)
    whole_l = lm.copy(); whole_l[1024:2048] = True                                        # a whole missing tile
    for name, a, b in (("left", lm, None), ("right", None, rm), ("both", lm, rm), ("tile", whole_l, rm), ("all_left", np.ones(len(lx), bool), rm),
                       ("all_right", lm, np.ones(len(rx), bool))):
        tl, tr = one_column(dfdb_mod, ctx, lx, a), one_column(dfdb_mod, ctx, rx, b)
        check_join(tl[dfdb_mod.ALL, "x"], lx, tr[dfdb_mod.ALL, "x"], rx, a, b, case=name)
        tl.close()
        tr.close()


def column_under(dfdb, t, spec, name):
    if spec is None:
        return t[dfdb.ALL, name]
    if spec[0] == "range":
        return t[dfdb.jr(spec[1], spec[2], dfdb.END), name]
    if spec[0] == "indices":
        return t[list(spec[1]), name]
    k = spec[3]
    return t[(spec[1], (lambda c: c < k) if spec[2] == "<" else (lambda c: c == k)), name]


@pytest.fixture(scope="module")
def two_tables(dfdb_mod, ctx):
    n = 20_001
    rng = np.random.default_rng(n)
    k = rng.integers(0, 4000, n).astype(np.int64)
    u = rng.integers(0, 100, n).astype(np.int64)
    tt = (np.arange(n) // 3000).astype(np.int64)
    big = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    for name, v in (("k", k), ("u", u), ("t", tt)):
        add_raw(dfdb_mod, big, name, v)
    p = rng.integers(0, 4000, 3000).astype(np.int64)
    small = one_column(dfdb_mod, ctx, p, name="k")
    return big, k, u, tt, small, p


def test_selections_on_either_side(dfdb_mod, ctx, two_tables):
    big, k, u, tt, small, p = two_tables
    sels = K.selections(u, tt)
    for name in ("none", "range", "indices", "pred10", "nothing", "empty_tiles"):
        spec, rows = sels[name]
        check_join(column_under(dfdb_mod, big, spec, "k"), k, small[dfdb_mod.ALL, "k"], p, lrows=rows, case=("left", name))
        check_join(small[dfdb_mod.ALL, "k"], p, column_under(dfdb_mod, big, spec, "k"), k, rrows=rows, case=("right", name))
    spec, rows = sels["pred10"]
    spec2, rows2 = sels["empty_tiles"]
    check_join(column_under(dfdb_mod, big, spec, "k"), k, column_under(dfdb_mod, big, spec2, "k"), k, lrows=rows, rrows=rows2, case="self-join, two views")
    col = column_under(dfdb_mod, big, spec2, "k")
    check_join(col, k, col, k, lrows=rows2, rrows=rows2, case="self-join, one query")


def test_row_bases(dfdb_mod, ctx):
    left, right = np.arange(2000, dtype=np.int64) % 700, np.arange(900, dtype=np.int64)
    tl, tr = one_column(dfdb_mod, ctx, left), one_column(dfdb_mod, ctx, right)
    add_raw(dfdb_mod, tl, "u", np.arange(2000, dtype=np.int64) % 3)
    tl.set_row_base(1 << 33)                                                               # (a leading range stage would number global rows: a predicate selects)
    tr.set_row_base(65536 * 5)
    check_join(tl[("u", lambda u: u == 1), "x"], left, tr[dfdb_mod.ALL, "x"], right, lrows=np.arange(1, 2000, 3), lbase=1 << 33, rbase=65536 * 5)
    tl.close()
    tr.close()


@pytest.fixture(scope="module")
def frames(dfdb_mod, ctx):
    import pandas as pd
    rng = np.random.default_rng(77)
    nl, nr = 3000, 500
    left = pd.DataFrame({"k": rng.integers(0, 600, nl).astype(np.int64), "a": rng.standard_normal(nl), "s": [f"row{i % 97}" + "x" * (i % 11) for i in range(nl)]})
    right = pd.DataFrame({"k": rng.integers(0, 600, nr).astype(np.int64), "b": rng.integers(-5, 5, nr).astype(np.int32), "name": [f"r{i}" for i in range(nr)]})
    tl = dfdb_mod.DFTable.from_columns({c: (left[c].tolist() if isinstance(left[c].iloc[0], str) else left[c].to_numpy()) for c in left}, ctx=ctx)
    tr = dfdb_mod.DFTable.from_columns({c: (right[c].tolist() if isinstance(right[c].iloc[0], str) else right[c].to_numpy()) for c in right}, ctx=ctx)
    return tl, left, tr, right


def frame_equal(got, want):
    assert list(got.columns) == list(want.columns) and len(got) == len(want), (list(got.columns), len(got), len(want))
    for c in want.columns:
        assert got[c].tolist() == want[c].tolist(), c


def test_device_lists_feed_the_gathers(dfdb_mod, ctx, frames):
    import torch
    tl, left, tr, right = frames
    v, w = tl[dfdb_mod.ALL, dfdb_mod.ALL], tr[("b", lambda b: b < 3), dfdb_mod.ALL]
    rsel = right[right["b"] < 3]
    ql = v._query()
    n, info = ql.join_count(w._query(), 0, 0, dfdb_mod.JOIN_INNER)
    wl, wr, _ = J.join_ref(left["k"].to_numpy(), None, None, right["k"].to_numpy(), None, np.flatnonzero((right["b"] < 3).to_numpy()), "inner")
    assert n == len(wl) and info[:4] == (len(left), len(rsel), 0, 0)
    w._q = None                                                                           # the right query is freed between call 1 and the fetch
    buf = torch.full((2, n + 2), SENTINEL, dtype=torch.int64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    for _ in range(2):                                                                    # and the fetch is repeated
        ql.join_fetch(n, (buf[0].data_ptr() + 8, buf[1].data_ptr() + 8))
        ctx.synchronize()
        h = buf.cpu().numpy()
        assert np.all(h[:, 0] == SENTINEL) and np.all(h[:, -1] == SENTINEL) and np.array_equal(h[0, 1:-1], wl) and np.array_equal(h[1, 1:-1], wr)
    lcols = ql.gather_rows_any(dev_ptr=buf[0].data_ptr() + 8, n=n)                        # the rows never leave the device; `s` is a String payload
    assert np.array_equal(lcols[0], left["k"].to_numpy()[wl - 1]) and np.array_equal(K.bits_of(lcols[1]), K.bits_of(left["a"].to_numpy()[wl - 1]))
    from dfdb.api import _flat_to_strings
    assert _flat_to_strings(*lcols[2]) == left["s"].to_numpy()[wl - 1].tolist()
    rcols = tr[dfdb_mod.ALL, dfdb_mod.ALL]._query().gather_rows_any(dev_ptr=buf[1].data_ptr() + 8, n=n)
    assert np.array_equal(rcols[1], right["b"].to_numpy()[wr - 1]) and _flat_to_strings(*rcols[2]) == right["name"].to_numpy()[wr - 1].tolist()
    lt, rt, info2 = ql.join(tr[dfdb_mod.ALL, dfdb_mod.ALL]._query(), 0, 0, dfdb_mod.JOIN_SEMI, device=True)
    ctx.synchronize()
    ws = J.join_ref(left["k"].to_numpy(), None, None, right["k"].to_numpy(), None, None, "semi")
    assert np.array_equal(lt.cpu().numpy(), ws[0]) and np.array_equal(rt.cpu().numpy(), ws[1]) and info2[:4] == ws[2]


def test_frames_against_pandas_merge(dfdb_mod, ctx, frames):
    tl, left, tr, right = frames
    v, w = tl[("a", lambda a: a < 0.5), dfdb_mod.ALL], tr[dfdb_mod.ALL, dfdb_mod.ALL]
    lsel = left[left["a"] < 0.5]
    frame_equal(dfdb_mod.innerjoin(v, w, "k"), lsel.merge(right, on="k", how="inner", sort=False))
    has = lsel["k"].isin(right["k"])
    frame_equal(dfdb_mod.semijoin(v, w, "k"), lsel[has])
    frame_equal(dfdb_mod.antijoin(v, w, "k"), lsel[~has])
    w2 = tr[dfdb_mod.ALL, ["name", "k"]]                                                   # on = (left name, right name); the right key is dropped where it stands
    frame_equal(dfdb_mod.innerjoin(v, w2, ("k", "k")), lsel.merge(right[["name", "k"]], on="k", how="inner", sort=False)[["k", "a", "s", "name"]])
    gl, gr, info = dfdb_mod.join_rows(v, w, "k", kind="left")
    wl, wr, winfo = J.join_ref(left["k"].to_numpy(), None, np.flatnonzero((left["a"] < 0.5).to_numpy()), right["k"].to_numpy(), None, None, "left")
    assert np.array_equal(gl, wl) and np.array_equal(gr, wr) and info[:4] == winfo
    with pytest.raises(ValueError, match="Duplicate variable names: a"):                   # a non-key name present on both sides (a self-join of the table)
        dfdb_mod.innerjoin(tl[dfdb_mod.ALL, ["k", "a"]], tl[dfdb_mod.ALL, ["k", "a"]], "k")
    with pytest.raises(ValueError, match="join kind"):
        dfdb_mod.join_rows(v, w, "k", kind="outer")
    with pytest.raises(KeyError):
        dfdb_mod.join_rows(v, w, "nope")


def test_matchmissing(dfdb_mod, ctx):
    (lx, lm), (rx, rm) = J.nullable_side(500, 1), J.nullable_side(300, 2)
    tl, tr, tp = one_column(dfdb_mod, ctx, lx, lm), one_column(dfdb_mod, ctx, rx, rm), one_column(dfdb_mod, ctx, rx)
    for a, b in ((tl, tp), (tp, tr), (tl, tr)):
        with pytest.raises(ValueError, match="missing values in the key column"):
            dfdb_mod.join_rows(a, b, "x")
    gl, gr, info = dfdb_mod.join_rows(tl, tr, "x", matchmissing="notequal")
    wl, wr, winfo = J.join_ref(lx, lm, None, rx, rm, None, "inner")
    assert np.array_equal(gl, wl) and np.array_equal(gr, wr) and info[:4] == winfo and winfo[2] == 100 and winfo[3] == 60
    for t in (tl, tr, tp):
        t.close()


def test_the_2_to_32_boundary(dfdb_mod, ctx):
    """1024 consecutive left rows may have 2^32 - 1 pairs between them and no more: call 1 only, nothing is fetched"""
    tl = one_column(dfdb_mod, ctx, np.full(1024, 9, np.int64))
    for nr, ok in ((4_194_303, True), (4_194_304, False)):
        tr = one_column(dfdb_mod, ctx, np.full(nr, 9, np.int64))
        ql, qr = tl[dfdb_mod.ALL, "x"].view._query(), tr[dfdb_mod.ALL, "x"].view._query()
        if ok:
            n, info = ql.join_count(qr, 0, 0, dfdb_mod.JOIN_INNER)
            assert n == (1 << 32) - 1024 and info == (1024, nr, 0, 0, 0)                  # an all-equal right side sorts in 0 passes
            assert ql.join_count(qr, 0, 0, dfdb_mod.JOIN_SEMI)[0] == 1024 and ql.join_count(qr, 0, 0, dfdb_mod.JOIN_ANTI)[0] == 0
        else:
            with pytest.raises(NotImplementedError, match=r"more than 2\^32 - 1 pairs from 1024 consecutive left rows"):
                ql.join_count(qr, 0, 0, dfdb_mod.JOIN_INNER)
            with pytest.raises(ValueError, match="dfdb_query_join has not been called"):   # the refused call left nothing pending
                ql.join_fetch(0)
            assert ql.join_count(qr, 0, 0, dfdb_mod.JOIN_SEMI)[0] == 1024                 # the other kinds of the same sides fit
        tr.close()
    tl.close()


def raw_join(ql, qr, lc, rc, kind):
    """the raw call with sentinel-filled outputs: (status, npairs, info)"""
    from dfdb import _native as N
    n = C.c_int64(SENTINEL)
    info = np.full(5, SENTINEL, np.int64)
    rc_ = N.load().dfdb_query_join(ql._h, lc, qr._h, rc, kind, C.byref(n), info.ctypes.data)
    return rc_, n.value, info


def test_refusals_name_the_form_and_touch_nothing(dfdb_mod, ctx, tmp_path):
    from dfdb import _native as N
    x = (np.arange(5000, dtype=np.int64) * 7919) % 1009
    t = one_column(dfdb_mod, ctx, x)
    t.add_column("s", ["a", "b", "c", "d"] * 1250)
    add_raw(dfdb_mod, t, "f", x.astype(np.float64))
    add_raw(dfdb_mod, t, "i", x.astype(np.int32))
    good = t[dfdb_mod.ALL, "x"].view._query()
    for lcol, rcol, pattern in ((t[dfdb_mod.ALL, "s"], t[dfdb_mod.ALL, "x"], "joining on a String column"), (t[dfdb_mod.ALL, "x"], t[dfdb_mod.ALL, "s"], "joining on a String column"),
                                (t[dfdb_mod.ALL, "x"] + 1, t[dfdb_mod.ALL, "x"], "joining on a computed column"), (t[dfdb_mod.ALL, "x"], t[dfdb_mod.ALL, "x"] + 1, "joining on a computed column"),
                                (t[dfdb_mod.ALL, "x"], t[dfdb_mod.ALL, "f"], "Int64 and Float64"), (t[dfdb_mod.ALL, "i"], t[dfdb_mod.ALL, "x"], "Int32 and Int64")):
        rc, n, info = raw_join(lcol.view._query(), rcol.view._query(), 0, 0, 0)
        assert rc == N.ERR_UNSUPPORTED and pattern in N.last_error() and n == SENTINEL and np.all(info == SENTINEL), (pattern, rc, N.last_error())
    for kind in (-1, 4, 99):
        rc, n, info = raw_join(good, good, 0, 0, kind)
        assert rc == N.ERR_ARGUMENT and "join kind" in N.last_error() and n == SENTINEL and np.all(info == SENTINEL)
    for lc, rc_col in ((1, 0), (0, -1)):
        rc, n, info = raw_join(good, good, lc, rc_col, 0)
        assert rc == N.ERR_BOUNDS and n == SENTINEL and np.all(info == SENTINEL)
    other = dfdb_mod.Context(0)                                                            # queries of two contexts
    t2 = one_column(dfdb_mod, other, x)
    rc, n, info = raw_join(good, t2[dfdb_mod.ALL, "x"].view._query(), 0, 0, 0)
    assert rc == N.ERR_ARGUMENT and "different contexts" in N.last_error() and n == SENTINEL and np.all(info == SENTINEL)
    # the fetch: nothing pending, then a capacity below the pairs — neither output is touched
    lr, rr = np.full(8000, SENTINEL, np.int64), np.full(8000, SENTINEL, np.int64)
    fresh = t[dfdb_mod.jr(1, 2, dfdb_mod.END), "x"].view._query()
    L = N.load()
    assert L.dfdb_query_join_fetch(fresh._h, lr.ctypes.data, rr.ctypes.data, 8000, N.MEM_HOST) == N.ERR_ARGUMENT and "has not been called" in N.last_error()
    n, info = fresh.join_count(good, 0, 0, dfdb_mod.JOIN_LEFT)
    assert n > 2500 and info[:2] == (2500, 5000)
    assert L.dfdb_query_join_fetch(fresh._h, lr.ctypes.data, rr.ctypes.data, n - 1, N.MEM_HOST) == N.ERR_BOUNDS and "BoundsError" in N.last_error()
    assert np.all(lr == SENTINEL) and np.all(rr == SENTINEL)
    gl, gr = fresh.join_fetch(n)                                                           # the refused fetch left the join pending
    wl, wr, _ = J.join_ref(x, None, np.arange(0, 5000, 2), x, None, None, "left")
    assert np.array_equal(gl, wl) and np.array_equal(gr, wr)
    gl2, none = fresh.join_fetch(n, want_right=False)                                      # a null right_rows is skipped
    assert none is None and np.array_equal(gl2, wl)
    fresh.reset()                                                                          # dfdb_query_reset drops the state
    assert L.dfdb_query_join_fetch(fresh._h, lr.ctypes.data, rr.ctypes.data, 8000, N.MEM_HOST) == N.ERR_ARGUMENT
    assert np.all(lr == SENTINEL) and np.all(rr == SENTINEL)
    # a view that is out of core: the table's files, opened without loading
    t.save(str(tmp_path / "tb"))
    tf = dfdb_mod.open_table(str(tmp_path / "tb"), ctx=ctx, load=False)
    for a, b in ((tf[dfdb_mod.ALL, "x"], t[dfdb_mod.ALL, "x"]), (t[dfdb_mod.ALL, "x"], tf[dfdb_mod.ALL, "x"])):
        rc, n, info = raw_join(a.view._query(), b.view._query(), 0, 0, 0)
        assert rc == N.ERR_UNSUPPORTED and "out of core" in N.last_error() and n == SENTINEL, N.last_error()
    tf.close()
    t.compress_column("x", 2)                                                              # what keep_compressed = 2 leaves: the LZ4 blocks alone
    rc, n, info = raw_join(t[dfdb_mod.ALL, "x"].view._query(), t[dfdb_mod.ALL, "x"].view._query(), 0, 0, 0)
    assert rc == N.ERR_UNSUPPORTED and "compressed-only" in N.last_error() and n == SENTINEL and np.all(info == SENTINEL)
    t2.close()
    other.close()
    t.close()


def test_a_table_of_2_to_31_rows_is_refused_on_either_side(dfdb_mod, ctx):
    """rows travel in 32 bits with the top bit spare: a table of 2^31 rows is refused by name on the left and on the right, before anything is launched (no
    selection is executed).  The column is generated on the device (17 GB, no host copy)"""
    from dfdb import _native as N
    big = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    big.add_generated("x", dfdb_mod.GEN_I64_IOTA, 0, 1 << 31)
    small = one_column(dfdb_mod, ctx, np.arange(100, dtype=np.int64))
    qb, qs = big[dfdb_mod.ALL, "x"].view._query(), small[dfdb_mod.ALL, "x"].view._query()
    for ql, qr, side in ((qb, qs, "left"), (qs, qb, "right"), (qb, qb, "left")):
        rc, n, info = raw_join(ql, qr, 0, 0, 0)
        assert rc == N.ERR_UNSUPPORTED and "joining a table of 2^31 rows or more (the %s side)" % side in N.last_error(), (side, rc, N.last_error())
        assert n == SENTINEL and np.all(info == SENTINEL), side
    lr = np.full(4, SENTINEL, np.int64)
    assert N.load().dfdb_query_join_fetch(qs._h, lr.ctypes.data, None, 4, N.MEM_HOST) == N.ERR_ARGUMENT and np.all(lr == SENTINEL)      # nothing is pending
    del qb
    big.close()
    small.close()


def counted(ctx, names, call):
    ctx.synchronize()
    ctx.profile(True)
    try:
        got = call()
        ctx.synchronize()
        return got, {k: ctx.profile_get(k)[0] for k in names}
    finally:
        ctx.profile(False)


def test_launch_counts_from_the_profile(dfdb_mod, ctx):
    left = np.arange(5000, dtype=np.int64) % 3
    tl, tr = one_column(dfdb_mod, ctx, left), one_column(dfdb_mod, ctx, np.full(3000, 1, np.int64))
    ql, qr = tl[dfdb_mod.ALL, "x"].view._query(), tr[dfdb_mod.ALL, "x"].view._query()
    assert (ql.count(), qr.count()) == (5000, 3000)
    names = ("join_probe", "join_expand", "sort_rows", "sort_build", "sort_count", "sort_scatter")
    (n, info), c = counted(ctx, names, lambda: ql.join_count(qr, 0, 0, dfdb_mod.JOIN_INNER))
    assert n == 1667 * 3000 and info == (5000, 3000, 0, 0, 0)                             # an all-equal right side: no digit pass
    assert c == {"join_probe": 1, "join_expand": 0, "sort_rows": 1, "sort_build": 1, "sort_count": 0, "sort_scatter": 0}, c
    for want_right in (True, False):
        (gl, gr), c = counted(ctx, names, lambda: ql.join_fetch(n, want_right=want_right))
        assert c == {"join_probe": 0, "join_expand": 1, "sort_rows": 0, "sort_build": 0, "sort_count": 0, "sort_scatter": 0}, c
        assert np.array_equal(gl, np.repeat(np.arange(2, 5001, 3), 3000)) and (gr is None or np.array_equal(gr, np.tile(np.arange(1, 3001), 1667)))
    tl.close()
    tr.close()
