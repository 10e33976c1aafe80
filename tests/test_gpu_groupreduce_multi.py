"""groupreduce by a TUPLE of key columns with several reducers in one call (dfdb_query_groupreduce_n; the reference's signature,
src/tables/aggregate.jl:1-14: `groupreduce(view, by::Tuple{Vararg{Symbol}}; cols...)`, numbering the groups by first appearance of the key tuple).
Checked against a numpy restatement written here: each key's isequal image (one NaN, -0.0 apart from 0.0, missing as its own tag, strings as bytes),
groups in order of the first selected row that holds the tuple, exact counts and integer results, Float64 sums within n * eps * sum|x|, signbit on
minimum / maximum.  Every case runs over a filtered view."""
import ctypes as C
import math
import os
import shutil
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAN_BITS = np.uint64(0x7ff8000000000000)


def key_image(col):
    """-> (missing flags, uint64 image) of one key column (numpy array, masked array or list of str / None)"""
    if isinstance(col, list):
        codes, miss = {}, np.zeros(len(col), np.uint64)
        img = np.empty(len(col), np.uint64)
        for i, s in enumerate(col):
            if s is None:
                miss[i] = 1; img[i] = 0
            else:
                img[i] = codes.setdefault(s.encode(), len(codes))
        return miss, img
    miss = np.ma.getmaskarray(col).astype(np.uint64) if isinstance(col, np.ma.MaskedArray) else np.zeros(len(col), np.uint64)
    a = np.ma.getdata(col)
    if a.dtype.kind == "M":
        a = a.astype(np.int64)
    if a.dtype.kind == "f":
        img = a.astype(np.float64).view(np.uint64).copy(); img[np.isnan(a)] = NAN_BITS
    else:
        img = a.astype(np.int64).view(np.uint64).copy()
    img[miss == 1] = 0
    return miss, img


def order_image(v, op):
    if v.dtype.kind == "f":
        b = v.astype(np.float64).view(np.uint64)
        im = np.where(b >> np.uint64(63) == 1, ~b, b | np.uint64(1 << 63))
        im[np.isnan(v)] = np.uint64(0) if op == "min" else ~np.uint64(0)
        return im
    if v.dtype.kind == "u":
        return v.astype(np.uint64)
    return v.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)


def from_image(im, v_dtype):
    if v_dtype.kind == "f":
        nan = (im == 0) | (im == ~np.uint64(0))
        b = np.where(im >> np.uint64(63) == 1, im & ~np.uint64(1 << 63), ~im)
        out = b.view(np.float64).copy(); out[nan] = np.nan
        return out
    if v_dtype.kind == "u":
        return im
    return (im ^ np.uint64(1 << 63)).view(np.int64)


def fsum_groups(v, gid, ng):
    """per group, the exact sum of the Float64 values rounded once (math.fsum); NaN where the group holds a NaN or infinities of both signs"""
    order = np.argsort(gid, kind="stable")
    ends = np.cumsum(np.bincount(gid, minlength=ng))
    vs, out, lo = v[order].tolist(), np.empty(ng, np.float64), 0
    for g, hi in enumerate(ends.tolist()):
        try:
            out[g] = math.fsum(vs[lo:hi])
        except (ValueError, OverflowError):
            out[g] = float(np.sum(v[order][lo:hi]))
        lo = hi
    return out


def expect(keys, sel, reducers, exact_float_sums=False):
    """keys: list of key columns; sel: bool mask; reducers: {name: (values or None, stat)} -> (first rows, counts, {name: values});
    exact_float_sums: Float sums and means from math.fsum per group instead of a float64 running sum"""
    rows = np.flatnonzero(sel)
    if len(rows) == 0:
        return rows, np.zeros(0, np.int64), {nm: None for nm in reducers}
    parts = []
    for k in keys:
        m, im = key_image(k)
        parts += [m[rows], im[rows]]
    mat = np.stack(parts, axis=1)
    _, first, inv = np.unique(mat, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(first), np.int64); rank[order] = np.arange(len(first))
    gid = rank[inv]; ng = len(first)
    cnt = np.bincount(gid, minlength=ng)
    out = {}
    for nm, (vals, stat) in reducers.items():
        if stat == "count":
            out[nm] = cnt; continue
        v = vals[rows]
        if stat in ("sum", "mean"):
            acc = np.zeros(ng, np.float64 if v.dtype.kind == "f" else (np.uint64 if v.dtype.kind == "u" else np.int64))
            if exact_float_sums and v.dtype.kind == "f":
                acc = fsum_groups(v.astype(np.float64), gid, ng)
            else:
                np.add.at(acc, gid, v.astype(acc.dtype))
            out[nm] = acc if stat == "sum" else acc.astype(np.float64) / cnt
        else:
            im = np.full(ng, ~np.uint64(0) if stat == "min" else np.uint64(0), np.uint64)
            (np.minimum if stat == "min" else np.maximum).at(im, gid, order_image(v, stat))
            out[nm] = from_image(im, v.dtype)
    return rows[first[order]], cnt, out


def check_frame(df, by, keys, sel, reducers, tag="", exact_float_sums=False):
    first_rows, cnt, want = expect(keys, sel, reducers, exact_float_sums)
    assert list(df.columns) == [*by, "count", *reducers], (tag, list(df.columns))
    assert len(df) == len(cnt), (tag, len(df), len(cnt))
    assert np.array_equal(df["count"].to_numpy(), cnt), tag
    if len(cnt) == 0:
        return
    for b, k in zip(by, keys):                                   # the keys in group order: the key column at the groups' first rows, under isequal
        got = df[b]
        if isinstance(k, list):
            want_k = [k[r] for r in first_rows]
            got_k = [None if (x is None or (isinstance(x, float) and np.isnan(x))) else x for x in got.tolist()]
            assert got_k == want_k, (tag, b)
            continue
        gm = got.isna().to_numpy() if isinstance(k, np.ma.MaskedArray) else np.zeros(len(got), bool)     # (a NaN key is a value, not missing)
        wm, wi = key_image(k)
        wm, wi = wm[first_rows].astype(bool), wi[first_rows]
        assert np.array_equal(gm, wm), (tag, b)
        raw = np.ma.getdata(k)
        gv = np.asarray(got.to_numpy()[~gm]).astype(raw.dtype if raw.dtype.kind != "M" else np.int64)
        _, gi = key_image(gv)
        assert np.array_equal(gi, wi[~wm]), (tag, b)
    for nm, (vals, stat) in reducers.items():
        got = df[nm].to_numpy(); w = want[nm]
        if stat == "count":
            assert np.array_equal(got, cnt), (tag, nm)
        elif vals.dtype.kind == "f" and stat in ("sum", "mean"):
            absum = expect(keys, sel, {"a": (np.abs(vals), "sum")})[2]["a"]
            tol = cnt * np.finfo(np.float64).eps * absum / (cnt if stat == "mean" else 1) + 1e-300
            nan = np.isnan(w)                                         # (a group with a NaN sums to NaN)
            with np.errstate(invalid="ignore"):                       # (an infinite sum is met exactly: inf - inf has no distance)
                near = (np.abs(got - w) <= tol) | (got == w)
            assert np.array_equal(np.isnan(got), nan) and np.all(near[~nan]), (tag, nm)
        elif stat == "mean":
            assert np.allclose(got, w, rtol=1e-12, atol=0), (tag, nm)
        elif vals.dtype.kind == "f":
            assert np.array_equal(np.isnan(got), np.isnan(w)), (tag, nm)
            ok = ~np.isnan(w)
            assert np.array_equal(got[ok], w[ok]) and np.array_equal(np.signbit(got[ok]), np.signbit(w[ok])), (tag, nm)
        else:
            assert np.array_equal(got.astype(w.dtype), w), (tag, nm)


def value_columns(rng, n):
    vi = rng.integers(-10**15, 10**15, n).astype(np.int64)
    vi[rng.random(n) < 0.01] = np.iinfo(np.int64).max                 # sums wrap
    vu8 = rng.integers(0, 256, n).astype(np.uint8)
    v32 = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    vf = rng.normal(size=n) * 1e3
    vf[rng.random(n) < 0.02] = 0.0
    vf[rng.random(n) < 0.02] = -0.0
    vf[rng.random(n) < 0.0005] = np.nan
    return {"vi": vi, "vu8": vu8, "v32": v32, "vf": vf}


def all_reducers(vals):
    return {"n": (None, "count"), "si": (vals["vi"], "sum"), "mi": (vals["vi"], "min"), "xi": (vals["vi"], "max"),
            "su8": (vals["vu8"], "sum"), "xu8": (vals["vu8"], "max"), "s32": (vals["v32"], "sum"), "m32": (vals["v32"], "min"),
            "sf": (vals["vf"], "sum"), "mf": (vals["vf"], "min"), "xf": (vals["vf"], "max"), "af": (vals["vf"], "mean"), "ai": (vals["vi"], "mean")}


def col_of(reducers, vals):
    inv = {id(v): k for k, v in vals.items()}
    return {nm: (None if v is None else inv[id(v)], stat) for nm, (v, stat) in reducers.items()}


def run_case(dfdb, ctx, keys, by, n, seed, sel_frac=0.7, dict_col=None, reducers_fn=all_reducers, extra=None):
    rng = np.random.default_rng(seed)
    vals = value_columns(rng, n)
    a = rng.random(n)
    cols = {"a": a, **dict(zip(by, keys)), **vals}
    t = dfdb.DFTable.from_columns(cols, block_size=65536, ctx=ctx)
    try:
        if dict_col:
            assert t.build_dictionary(dict_col) > 0
        reds = reducers_fn(vals)
        for view, sel, tag in ((t[("a", lambda c: c < sel_frac), dfdb.ALL], a < sel_frac, "filtered"), (t[("a", lambda c: c > 2.0), dfdb.ALL], a > 2.0, "empty")):
            df = dfdb.groupreduce(view, tuple(by), **col_of(reds, vals))
            check_frame(df, by, keys, sel, reds, tag)
        if extra:
            extra(t, vals, a)
    finally:
        t.close()


def test_two_keys_int64_and_string(dfdb_mod, ctx):
    rng = np.random.default_rng(11)
    n = 300_017
    k1 = rng.integers(-20, 20, n).astype(np.int64)
    words = [f"brand-{i:03d}" + "x" * (i % 19) for i in range(40)]
    k2 = [None if rng.random() < 0.01 else words[i] for i in rng.integers(0, 40, n)]
    run_case(dfdb_mod, ctx, [k1, k2], ["k1", "k2"], n, 1)


def test_three_keys_nullable_float_uint8(dfdb_mod, ctx):
    rng = np.random.default_rng(12)
    n = 250_003
    k1 = np.ma.masked_array(rng.integers(0, 7, n).astype(np.int64) * 10**12, mask=rng.random(n) < 0.05)
    k2 = rng.integers(0, 5, n).astype(np.float64) / 2
    u = rng.random(n)
    k2[u < 0.05] = np.nan
    k2[(u >= 0.05) & (u < 0.1)] = -0.0
    k2[(u >= 0.1) & (u < 0.15)] = 0.0
    k3 = rng.integers(0, 4, n).astype(np.uint8)
    run_case(dfdb_mod, ctx, [k1, k2, k3], ["k1", "k2", "k3"], n, 2)


def test_dictionary_string_and_int32(dfdb_mod, ctx):
    rng = np.random.default_rng(13)
    n = 200_001
    brands = [f"b{i}" for i in range(12)]
    k1 = [brands[i] for i in rng.integers(0, 12, n)]
    k2 = rng.integers(-3, 30, n).astype(np.int32)
    run_case(dfdb_mod, ctx, [k1, k2], ["k1", "k2"], n, 3, dict_col="k1")


def test_date_key(dfdb_mod, ctx):
    rng = np.random.default_rng(14)
    n = 150_001
    k1 = (np.datetime64("2020-01-01") + rng.integers(0, 60, n).astype("timedelta64[D]")).astype("datetime64[D]")
    k2 = rng.integers(0, 3, n).astype(np.int64)
    rng2 = np.random.default_rng(15)
    vals = value_columns(rng2, n)
    a = rng2.random(n)
    t = dfdb_mod.DFTable.from_columns({"a": a, "d": k1, "k2": k2, **vals}, block_size=65536, ctx=ctx)
    try:
        v = t[("a", lambda c: c < 0.5), dfdb_mod.ALL]
        df = dfdb_mod.groupreduce(v, ("d", "k2"), s=("vi", "sum"), m=("vf", "max"))
        sel = a < 0.5
        days = k1.astype(np.int64)
        first_rows, cnt, want = expect([days, k2], sel, {"s": (vals["vi"], "sum"), "m": (vals["vf"], "max")})
        assert np.array_equal(df["count"].to_numpy(), cnt)
        got_days = np.asarray(df["d"].to_numpy()).astype("datetime64[D]").astype(np.int64) if df["d"].dtype.kind == "M" else np.asarray(df["d"].to_numpy(), np.int64) - 719163
        assert np.array_equal(got_days, days[first_rows])
        assert np.array_equal(df["k2"].to_numpy(), k2[first_rows])
        assert np.array_equal(df["s"].to_numpy(), want["s"])
        assert np.array_equal(df["m"].to_numpy(), want["m"], equal_nan=True)
    finally:
        t.close()


@pytest.mark.parametrize("size", ["one_row", "few", "over_10k", "million", "hot"])
def test_sizes(dfdb_mod, ctx, size):
    rng = np.random.default_rng(hash(size) % 1000)
    if size == "one_row":
        n = 1
        k1 = np.array([5], np.int64); k2 = np.array([-0.0])
    elif size == "few":
        n = 500_000
        k1 = rng.integers(0, 10, n).astype(np.int64); k2 = rng.integers(0, 9, n).astype(np.float64)
    elif size == "over_10k":
        n = 600_000
        k1 = rng.integers(0, 150, n).astype(np.int64) * 7_777_777; k2 = rng.integers(0, 200, n).astype(np.float64)
    elif size == "million":
        n = 4_000_000
        k1 = rng.integers(0, 2000, n).astype(np.int64) << 33; k2 = rng.integers(0, 1000, n).astype(np.float64) - 500
    else:                                                         # one tuple holds 30 % of the rows (the global form's hot slots)
        n = 3_000_000
        k1 = rng.integers(0, 400, n).astype(np.int64); k2 = rng.integers(0, 500, n).astype(np.float64)
        hot = rng.random(n) < 0.3
        k1[hot] = 17; k2[hot] = 3.5
    sel_frac = 2.0 if size == "one_row" else 0.9
    run_case(dfdb_mod, ctx, [k1, k2], ["k1", "k2"], n, 20, sel_frac=sel_frac,
             reducers_fn=lambda v: {"si": (v["vi"], "sum"), "xf": (v["vf"], "max"), "mf": (v["vf"], "min"), "n": (None, "count")})
    if size == "million":
        sel = np.ones(n, bool)
        assert len(expect([k1, k2], sel, {})[1]) > 900_000


def test_single_key_identity(dfdb_mod, ctx):
    """one key with several reducers: the same keys, order and counts as one dfdb.groupreduce(v, by, col, stat) per reducer, the same values (Float64 sums within
    the tolerance); one key with one reducer is handed to dfdb_query_groupreduce itself: bit-identical"""
    rng = np.random.default_rng(21)
    n = 400_003
    k = rng.integers(0, 3000, n).astype(np.int64) * 3
    ks = [f"s{i}" for i in rng.integers(0, 300, n)]
    vals = value_columns(rng, n)
    a = rng.random(n)
    t = dfdb_mod.DFTable.from_columns({"a": a, "k": k, "ks": ks, **vals}, block_size=65536, ctx=ctx)
    try:
        v = t[("a", lambda c: c < 0.8), dfdb_mod.ALL]
        for by in ("k", "ks"):
            reds = {"sum": ("vi", "sum"), "min": ("vf", "min"), "max": ("vu8", "max"), "mean": ("vf", "mean")}
            multi = dfdb_mod.groupreduce(v, (by,), **reds)
            for nm, (c, stat) in reds.items():
                one = dfdb_mod.groupreduce(v, by, c, stat)
                assert list(one[by]) == list(multi[by]) and np.array_equal(one["count"].to_numpy(), multi["count"].to_numpy())
                if stat in ("sum", "mean") and c == "vf":             # (Float64 sums: atomic adds in no fixed order)
                    assert np.allclose(multi[nm].to_numpy(), one[stat].to_numpy(), rtol=1e-9, atol=1e-9, equal_nan=True)
                else:
                    assert np.array_equal(multi[nm].to_numpy(), one[stat].to_numpy(), equal_nan=True)
            for c, stat in (("vf", "max"), ("vi", "min"), ("vu8", "sum"), ("vi", "sum")):
                one = dfdb_mod.groupreduce(v, by, c, stat)
                solo = dfdb_mod.groupreduce(v, (by,), x=(c, stat))
                assert list(one[by]) == list(solo[by]) and np.array_equal(one["count"].to_numpy(), solo["count"].to_numpy())
                assert one[stat].to_numpy().tobytes() == solo["x"].to_numpy().tobytes()
    finally:
        t.close()


def raw_call(dfdb, q, keys, vals, stats):
    """dfdb_query_groupreduce_n on a query handle -> (return code, ngroups)"""
    from dfdb import _native as N
    L = N.load()
    kc = (C.c_int32 * max(len(keys), 1))(*keys)
    vc = (C.c_int32 * max(len(vals), 1))(*vals)
    st = (C.c_int32 * max(len(stats), 1))(*stats)
    ng, kb = C.c_int64(), (C.c_int64 * 8)()
    return L.dfdb_query_groupreduce_n(q._h, kc, len(keys), vc, st, len(stats), C.byref(ng), kb), ng.value


def test_selection_restored_and_errors(dfdb_mod, ctx):
    from dfdb import api
    from dfdb import _native as N
    rng = np.random.default_rng(31)
    n = 100_000
    k1 = rng.integers(0, 50, n).astype(np.int64)
    k2 = rng.integers(0, 7, n).astype(np.int32)
    x = rng.normal(size=n)
    xn = np.ma.masked_array(rng.integers(0, 9, n).astype(np.int64), mask=rng.random(n) < 0.1)
    a = rng.random(n)
    t = dfdb_mod.DFTable.from_columns({"a": a, "k1": k1, "k2": k2, "x": x, "xn": xn}, block_size=65536, ctx=ctx)
    try:
        v = t[("a", lambda c: c < 0.3), ["k1", "k2", "x", "xn"]]
        q = api._Query(v)
        before_n, before_idx = q.count(), q.indices().copy()
        rc, ng = raw_call(dfdb_mod, q, [0, 1], [2, 2], [N.AGG_SUM, N.AGG_MAX])
        assert rc == N.OK and ng == len(np.unique(np.stack([k1[a < 0.3], k2[a < 0.3]], 1), axis=0))
        assert q.count() == ng                                   # between the call and its fetch: the groups' first rows
        outs = (N.OutCol * 2)()
        bufs = [np.empty(ng, np.int64), np.empty(ng, np.int32)]
        for i in range(2):
            outs[i].data = bufs[i].ctypes.data; outs[i].memkind = N.MEM_HOST
        cnt = np.empty(ng, np.int64); vi = np.empty(2 * ng, np.int64); vf = np.empty(2 * ng, np.float64)
        L = N.load()
        assert L.dfdb_query_groupreduce_n_fetch(q._h, outs, cnt.ctypes.data, vi.ctypes.data, vf.ctypes.data) == N.OK
        assert q.count() == before_n and np.array_equal(q.indices(), before_idx)
        assert cnt.sum() == before_n
        # a fetch without a call
        assert L.dfdb_query_groupreduce_n_fetch(q._h, outs, cnt.ctypes.data, vi.ctypes.data, vf.ctypes.data) == N.ERR_ARGUMENT
        assert raw_call(dfdb_mod, q, [], [], [])[0] == N.ERR_ARGUMENT                      # no key column
        assert raw_call(dfdb_mod, q, [0, 9], [], [])[0] == N.ERR_BOUNDS                     # a projection column that is not there
        assert raw_call(dfdb_mod, q, [0, 1], [7], [N.AGG_SUM])[0] == N.ERR_BOUNDS
        assert raw_call(dfdb_mod, q, [0, 1], [2], [9])[0] == N.ERR_ARGUMENT                 # unknown statistic
        assert raw_call(dfdb_mod, q, [0, 1], [3], [N.AGG_SUM])[0] == N.ERR_UNSUPPORTED      # a nullable value column
        assert q.count() == before_n and np.array_equal(q.indices(), before_idx)
        vc = t[("a", lambda c: c < 0.3), dfdb_mod.ALL]
        comp = dfdb_mod.map_to_column(lambda k: k * 2, vc[dfdb_mod.ALL, ["k1"]])
        qc = api._Query(api.DFView(t, api.Projection({"k2": vc.projection.cols["k2"], "kk": comp.expr}), vc.selection))
        assert raw_call(dfdb_mod, qc, [0, 1], [], [])[0] == N.ERR_UNSUPPORTED               # a computed key column
        with pytest.raises(ValueError):
            dfdb_mod.groupreduce(v, "k1", "x", "sum", s=("x", "sum"))
        with pytest.raises(ValueError):
            dfdb_mod.groupreduce(v, ("k1", "k2"), s=("x", "median"))
        # out of core each fetch takes only its own call's groups, also where the _n call has one key and one reducer; a refused fetch leaves them pending
        d = tempfile.mkdtemp(prefix="dfdb_grn_")
        try:
            t.save(os.path.join(d, "tb"))
            lazy = dfdb_mod.open_table(os.path.join(d, "tb"), load=False, ctx=ctx)
            try:
                ql = api._Query(lazy[("a", lambda c: c < 0.3), ["k1", "k2", "x", "xn"]])
                want = len(np.unique(k1[a < 0.3]))
                out1 = (N.OutCol * 1)()
                out1[0].data = bufs[0].ctypes.data; out1[0].memkind = N.MEM_HOST
                plain = lambda: L.dfdb_query_groupreduce_fetch(ql._h, out1, cnt.ctypes.data, vi.ctypes.data, vf.ctypes.data)   # noqa: E731
                multi = lambda: L.dfdb_query_groupreduce_n_fetch(ql._h, out1, cnt.ctypes.data, vi.ctypes.data, vf.ctypes.data)  # noqa: E731
                rc, ng1 = raw_call(dfdb_mod, ql, [0], [2], [N.AGG_SUM])
                assert rc == N.OK and ng1 == want and not lazy.resident(0)
                assert plain() == N.ERR_ARGUMENT
                assert multi() == N.OK and cnt[:ng1].sum() == before_n
                assert multi() == N.ERR_ARGUMENT                                           # the fetch cleared them
                ng2, kb2 = C.c_int64(), C.c_int64()
                assert L.dfdb_query_groupreduce(ql._h, 0, 2, N.AGG_SUM, C.byref(ng2), C.byref(kb2)) == N.OK and ng2.value == want
                assert multi() == N.ERR_ARGUMENT
                assert plain() == N.OK and cnt[:ng1].sum() == before_n
                assert plain() == N.ERR_ARGUMENT
                assert not lazy.resident(0)
            finally:
                lazy.close()
        finally:
            shutil.rmtree(d, ignore_errors=True)
    finally:
        t.close()


def test_out_of_core_equals_resident(dfdb_mod, ctx):
    rng = np.random.default_rng(41)
    n = 400_000
    k1 = rng.integers(0, 30, n).astype(np.int64)
    words = [f"w{i}" for i in range(25)]
    k2 = [words[i] for i in rng.integers(0, 25, n)]
    k3 = np.ma.masked_array(rng.integers(0, 3, n).astype(np.int16), mask=rng.random(n) < 0.1)
    vals = value_columns(rng, n)
    a = rng.random(n)
    t = dfdb_mod.DFTable.from_columns({"a": a, "k1": k1, "k2": k2, "k3": k3, **vals}, block_size=65536, ctx=ctx)
    d = tempfile.mkdtemp(prefix="dfdb_grn_")
    reds = {"n": (None, "count"), "s": ("vi", "sum"), "m": ("vf", "min"), "x": ("vf", "max"), "u": ("vu8", "sum"), "f": ("vf", "sum")}
    try:
        res = dfdb_mod.groupreduce(t[("a", lambda c: c < 0.6), dfdb_mod.ALL], ("k1", "k2", "k3"), **reds)
        t.save(os.path.join(d, "tb"))
        lazy = dfdb_mod.open_table(os.path.join(d, "tb"), load=False, ctx=ctx)
        ctx.set_option("ooc_chunk_blocks", 2)
        try:
            ooc = dfdb_mod.groupreduce(lazy[("a", lambda c: c < 0.6), dfdb_mod.ALL], ("k1", "k2", "k3"), **reds)
            assert not lazy.resident(0)
        finally:
            ctx.set_option("ooc_chunk_blocks", 512)
            lazy.close()
        assert list(ooc.columns) == list(res.columns) and len(ooc) == len(res)
        for c in ("k1", "k2", "n", "s", "m", "x", "u"):
            assert list(ooc[c]) == list(res[c]) or np.array_equal(ooc[c].to_numpy(), res[c].to_numpy(), equal_nan=True), c
        assert np.array_equal(ooc["k3"].isna().to_numpy(), res["k3"].isna().to_numpy())
        assert np.allclose(ooc["f"].to_numpy(), res["f"].to_numpy(), rtol=1e-9, atol=1e-6, equal_nan=True)     # (Float64 sums: chunk sums of atomic adds)
        check_frame(ooc, ["k1", "k2", "k3"], [k1, k2, k3], a < 0.6, {nm: (None if c is None else vals[c], st) for nm, (c, st) in reds.items()}, "ooc")
    finally:
        t.close()
        shutil.rmtree(d, ignore_errors=True)
