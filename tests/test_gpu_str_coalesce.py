"""coalesce(a, b) with a String result on the device (include/dfdb_ir.h DFIR_COALESCE; csrc/k_strings.hip K6, the filled forms): a String column leaf, then a string constant
or a second String column, as a whole projection column.  The yardstick is tests/str_coalesce_cases.py (pinned by tests/test_str_coalesce_cpu.py), applied to
the lists the columns were made of; every comparison is bit-exact: the sizes array (-1 for missing), the byte arena, the string-bytes total and the count."""
import ctypes as C

import numpy as np
import pytest

import str_coalesce_cases as K
from str_coalesce_cases import coalesce_ref, flat, unflat

pytestmark = pytest.mark.gpu
BS, N = 4096, K.N
PATTERNS = list(K.missing_patterns())
CATS = [b"x", b"yy", b"x", b"", b"zzz-long-one", b"x", b"q\xc3\xa9"]          # a low-cardinality column: a dictionary can be built on it


class Data:
    def __init__(self):
        self.rows = K.row_strings()
        self.k = np.arange(N, dtype=np.int64)
        self.cols = {"a_" + n: K.with_missing(self.rows, m) for n, m in K.missing_patterns().items()}
        self.cols["p"] = self.rows                                                # a plain String column
        self.cols["bp"], self.cols["bn"] = K.default_columns()
        self.cols["cp"] = [CATS[(i * 3 + i // 50) % len(CATS)] for i in range(N)]  # plain, low cardinality
        self.cols["cn"] = K.with_missing(self.cols["cp"], self.k % 5 == 2)
        self.nullable = {n: n.startswith("a_") or n in ("bn", "cn") for n in self.cols}


@pytest.fixture(scope="module")
def data():
    return Data()


def make_table(dfdb, data, ctx=None, block_size=BS):
    from dfdb import ir
    t = dfdb.DFTable.new(block_size=block_size, ctx=ctx)
    for name, vals in data.cols.items():
        t.add_column(name, list(vals), dtype=ir.STRING | (ir.NULLABLE if data.nullable[name] else 0))
    t.add_column("k", data.k)
    return t


@pytest.fixture(scope="module")
def table(dfdb_mod, ctx, data):
    t = make_table(dfdb_mod, data)
    yield t
    t.close()


def string_bytes(q, i=0):
    from dfdb import _native as NAT
    nb = C.c_int64(-1)
    NAT.check(NAT.load().dfdb_result_string_bytes(q._h, i, C.byref(nb)))
    return nb.value


def project(dfdb, t, a, b):
    """the projector of coalesce(a, b): b a column name or a bytes constant"""
    from dfdb import ir
    if isinstance(b, bytes):
        return {"r": (a, lambda x: ir.coalesce(x, b))}
    return {"r": ((a, b), lambda x, y: ir.coalesce(x, y))}


def check(dfdb, t, want, view):
    """string bytes before materializing, then count, sizes and arena of projection column `r` (the last one)"""
    ws, wd, wt = flat(want)
    q = view._query()
    i = len(view.projection) - 1
    assert q.count() == len(want)
    assert string_bytes(q, i) == wt
    sizes, arena = q.materialize()[i]
    assert sizes.dtype == np.int32 and np.array_equal(sizes, ws), (np.nonzero(sizes != ws)[0][:5], len(sizes), len(ws))
    assert len(arena) == wt and np.array_equal(arena, wd)
    return q


def expected(data, a, b, mask=None):
    full = coalesce_ref(data.cols[a], b if isinstance(b, bytes) else data.cols[b])
    return full if mask is None else [v for v, m in zip(full, mask) if m]


# ---------------------------------------------------------------- typing and refusals
def test_result_type(dfdb_mod, ctx, table):
    from dfdb import ir
    o = table.ordinal
    a, p, bp, bn = ir.col(o("a_every7th")), ir.col(o("p")), ir.col(o("bp")), ir.col(o("bn"))
    assert table.expr_dtype(ir.coalesce(a, "x")) == ir.STRING and table.expr_dtype(ir.coalesce(p, "")) == ir.STRING
    assert table.expr_dtype(ir.coalesce(a, bp)) == ir.STRING
    assert table.expr_dtype(ir.coalesce(a, bn)) == ir.STRING | ir.NULLABLE and table.expr_dtype(ir.coalesce(p, bn)) == ir.STRING | ir.NULLABLE
    assert table.expr_dtype(ir.coalesce(a, a)) == ir.STRING | ir.NULLABLE
    assert table.expr_dtype(ir.coalesce(a, b"c" * 65535)) == ir.STRING            # the longest constant taken
    assert table.expr_logical(ir.coalesce(a, "x")) == ""
    assert table.expr_dtype(ir.coalesce(ir.col(o("k")), 5)) == ir.I64             # the numeric coalesce is what it was


def test_refusals(dfdb_mod, ctx, table):
    from dfdb import ir
    o = table.ordinal
    a, bn, k = ir.col(o("a_every7th")), ir.col(o("bn")), ir.col(o("k"))
    sc = ir.coalesce(a, "x")
    operands = [sc == "y", sc == a, a < sc, ir.sizeof(sc), ir.parse(ir.I64, sc), ir.datetime19(sc), ir.startswith(sc, "x"), ir.endswith(sc, "x"),
                ir.ismissing(sc), ir.coalesce(sc, "y"), ir.coalesce(a, sc), ir.coalesce(sc == "y", False)]
    for e in operands:
        with pytest.raises(NotImplementedError, match="whole projection column"):
            table.expr_dtype(e)
    for e in (ir.coalesce(ir.const("c"), a), ir.coalesce(ir.const("c"), ir.const("d"))):          # a is no column leaf
        with pytest.raises(NotImplementedError, match="takes a String column"):
            table.expr_dtype(e)
    for e in (ir.coalesce(a, 5), ir.coalesce(a, k), ir.coalesce(k, "x"), ir.coalesce(a, ir.sizeof(bn))):
        with pytest.raises(NotImplementedError, match="the result would be a Union of two value types"):
            table.expr_dtype(e)
    with pytest.raises(NotImplementedError, match="at most 65535"):
        table.expr_dtype(ir.coalesce(a, b"c" * 65536))
    with pytest.raises(NotImplementedError, match="not as a predicate"):                          # as a predicate, straight at the ABI
        dfdb_mod.DFView(table, None, dfdb_mod.SelectionQueue((sc,)))._query()
    v = dfdb_mod.DFView(table)
    with pytest.raises(NotImplementedError, match="unique of a computed column: materialise it as a column first"):
        dfdb_mod.coalesce(v.a_every7th, "x").unique()
    with pytest.raises(NotImplementedError, match="groupreduce by a computed column: materialise it as a column first"):
        dfdb_mod.groupreduce(v[dfdb_mod.ALL, {"r": ("a_every7th", lambda x: ir.coalesce(x, "x")), "k": "k"}], "r", "k", "sum")


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_missing_pattern_against_every_default(dfdb_mod, ctx, table, data, pattern):
    a = "a_" + pattern
    v = dfdb_mod.DFView(table)
    for b in K.CONSTANTS + ["bp", "bn"]:
        check(dfdb_mod, table, expected(data, a, b), v[dfdb_mod.ALL, project(dfdb_mod, table, a, b)])


def test_all_missing_with_the_empty_constant_has_no_bytes(dfdb_mod, ctx, table, data):
    q = check(dfdb_mod, table, [b""] * N, dfdb_mod.DFView(table)[dfdb_mod.ALL, project(dfdb_mod, table, "a_all", b"")])
    assert string_bytes(q) == 0


def test_a_non_nullable_a_gives_the_column_back(dfdb_mod, ctx, table, data):
    v = dfdb_mod.DFView(table)
    for b in (b"never taken", "bn", "bp"):
        check(dfdb_mod, table, data.rows, v[dfdb_mod.ALL, project(dfdb_mod, table, "p", b)])
    plain = v[dfdb_mod.ALL, ["p"]]._query().materialize()[0]
    got = v[dfdb_mod.ALL, project(dfdb_mod, table, "p", b"never taken")]._query().materialize()[0]
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1])


def test_string_is_coalesce_with_missing(dfdb_mod, ctx, table, data):
    v = dfdb_mod.DFView(table)
    c = dfdb_mod.string(v.a_every7th)
    assert c.expr.same(dfdb_mod.coalesce(v.a_every7th, "missing").expr) and c.eltype == dfdb_mod.ir.STRING
    check(dfdb_mod, table, expected(data, "a_every7th", b"missing"), c.view)
    assert dfdb_mod.string(v.p) is v.p or dfdb_mod.string(v.p).expr.same(v.p.expr)              # a plain String column: the column itself
    with pytest.raises(NotImplementedError):
        dfdb_mod.string(v.k)
    got = dfdb_mod.materialize(c)                                                               # like any String column: one str (or None) per row
    want = [x.decode(errors="replace") for x in expected(data, "a_every7th", b"missing")]
    assert got.dtype == object and list(got) == want


SELECTIONS = ["range", "indices", "predicate", "empty"]


def selection_of(dfdb, data, name, table):
    """(selector, mask)"""
    from dfdb import ir
    k = data.k
    if name == "range":
        m = np.zeros(N, bool); m[99:3000:3] = True
        return dfdb.jr(100, 3, 3000), m
    if name == "indices":
        rows = np.unique(np.concatenate(([0, 63, 64, 1023, 1024, 2047, 2048, N - 1], np.random.default_rng(5).integers(0, N, 200))))
        m = np.zeros(N, bool); m[rows] = True
        return (rows + 1).tolist(), m
    if name == "predicate":
        return ir.col(table.ordinal("k")) % 10 == 3, k % 10 == 3
    return ir.col(table.ordinal("k")) < 0, np.zeros(N, bool)


@pytest.mark.parametrize("sel", SELECTIONS)
def test_selections(dfdb_mod, ctx, table, data, sel):
    s, m = selection_of(dfdb_mod, data, sel, table)
    v = dfdb_mod.DFView(table)[s, dfdb_mod.ALL]
    for a, b in (("a_every7th", b"missing"), ("a_run-over-boundary", b""), ("a_tile2", "bn"), ("a_every7th", "bp"), ("a_all", "bn"), ("a_every7th", "cp")):
        check(dfdb_mod, table, expected(data, a, b, m), v[dfdb_mod.ALL, project(dfdb_mod, table, a, b)])


@pytest.mark.parametrize("dictionary", [False, True], ids=["flat", "dictionary"])
def test_the_shortcuts_of_a_plain_projection_do_not_leak(dfdb_mod, ctx, data, dictionary):
    """coalesce(c == "x", false) on the coalesced column itself with hint_materialize (check() materializes, which sets it): K5 may capture the selected rows of
    c, and "every selected row of c holds x" is known — both answer for c's rows only.  Alone, beside c projected plainly, as the second side, and with a
    dictionary on the plain column"""
    from dfdb import ir
    t = make_table(dfdb_mod, data)
    try:
        if dictionary:
            assert t.build_dictionary("cp") == len(set(CATS))
        v = dfdb_mod.DFView(t)
        for c in ("cn", "cp"):
            for pat, op in ((b"x", "eq"), (b"x", "ne"), (b"zzz-long-one", "eq")):
                oc = t.ordinal(c)
                term = (ir.col(oc) == pat) if op == "eq" else (ir.col(oc) != pat)
                m = np.array([x is not None and ((x == pat) == (op == "eq")) for x in data.cols[c]])
                sv = v[ir.coalesce(term, False), dfdb_mod.ALL]
                check(dfdb_mod, t, expected(data, c, b"dflt", m), sv[dfdb_mod.ALL, project(dfdb_mod, t, c, b"dflt")])
                both = sv[dfdb_mod.ALL, {"plain": c, "r": (c, lambda x: ir.coalesce(x, b"dflt"))}]
                q = check(dfdb_mod, t, expected(data, c, b"dflt", m), both)
                ps, pd = q.materialize()[0]
                ws, wd, _ = flat([x for x, k in zip(data.cols[c], m) if k])
                assert np.array_equal(ps, ws) and np.array_equal(pd, wd)
                check(dfdb_mod, t, expected(data, "a_every7th", c, m), sv[dfdb_mod.ALL, project(dfdb_mod, t, "a_every7th", c)])       # c as the second side
        check(dfdb_mod, t, expected(data, "cp", b"never"), v[dfdb_mod.ALL, project(dfdb_mod, t, "cp", b"never")])
        check(dfdb_mod, t, expected(data, "cn", "cp"), v[dfdb_mod.ALL, project(dfdb_mod, t, "cn", "cp")])
    finally:
        t.close()


def test_host_and_device_outputs_and_a_short_arena(dfdb_mod, ctx, table, data):
    import torch
    from dfdb import _native as NAT
    L = NAT.load()
    dev = torch.device("cuda", 0)
    for a, b in (("a_every7th", b"seventeen bytes !"), ("a_every7th", "bn")):
        want = expected(data, a, b)
        ws, wd, wt = flat(want)
        q = dfdb_mod.DFView(table)[dfdb_mod.ALL, project(dfdb_mod, table, a, b)]._query()
        assert q.count() == N and string_bytes(q) == wt
        sizes = torch.full((N,), -7, dtype=torch.int32, device=dev)
        arena = torch.zeros(wt + 64, dtype=torch.uint8, device=dev)
        outs = (NAT.OutCol * 1)()
        outs[0].data, outs[0].memkind, outs[0].bytes, outs[0].bytes_cap = sizes.data_ptr(), NAT.MEM_DEVICE, arena.data_ptr(), wt
        NAT.check(L.dfdb_materialize(q._h, outs, 1))
        torch.cuda.synchronize()
        assert outs[0].count == N and outs[0].nbytes == wt and outs[0].dtype == q.coltype(0)
        assert np.array_equal(sizes.cpu().numpy(), ws) and np.array_equal(arena.cpu().numpy()[:wt], wd)
        assert not arena.cpu().numpy()[wt:].any()                                       # nothing written behind the arena
        for kind in (NAT.MEM_DEVICE, NAT.MEM_HOST):                                     # one byte short: the existing DFDB_ERR_ARGUMENT
            hs, hb = np.empty(N, np.int32), np.empty(wt, np.uint8)
            outs[0].memkind, outs[0].bytes_cap = kind, wt - 1
            if kind == NAT.MEM_HOST:
                outs[0].data, outs[0].bytes = hs.ctypes.data, hb.ctypes.data
            with pytest.raises(ValueError, match=f"needs {wt} string bytes, capacity is {wt - 1}"):
                NAT.check(L.dfdb_materialize(q._h, outs, 1))
        outs[0].bytes_cap = wt                                                          # and the host output through the ABI
        NAT.check(L.dfdb_materialize(q._h, outs, 1))
        assert np.array_equal(hs, ws) and np.array_equal(hb, wd) and outs[0].nbytes == wt


# ---------------------------------------------------------------- add_column!
def strs(values):
    return [None if v is None else v.decode(errors="replace") for v in values]


def test_add_column_from_makes_a_column_like_a_loaded_one(oracle, dfdb_mod, ctx, data, tmp_path):
    from dfdb import ir
    t = make_table(dfdb_mod, data)
    t2 = dfdb_mod.DFTable.new(block_size=BS)
    try:
        v = dfdb_mod.DFView(t)
        # into the view's own table: a constant default (String) and a nullable second side (Union{String,Missing})
        t.add_column_from("r_const", v[dfdb_mod.ALL, project(dfdb_mod, t, "a_every7th", b"missing")])
        t.add_column_from("r_null", dfdb_mod.coalesce(v.a_tile2, v.bn))
        t.add_column_from("r_cat", dfdb_mod.coalesce(v.cn, "x"))
        assert t.getmeta("r_const").type == "String" and t.getmeta("r_null").type == "Missing(String)" and t.getmeta("r_cat").type == "String"
        want = {"r_const": expected(data, "a_every7th", b"missing"), "r_null": expected(data, "a_tile2", "bn"), "r_cat": expected(data, "cn", b"x")}
        v = dfdb_mod.DFView(t)
        for name, w in want.items():
            ws, wd, _ = flat(w)
            sizes, arena = v[dfdb_mod.ALL, [name]]._query().materialize()[0]
            assert np.array_equal(sizes, ws) and np.array_equal(arena, wd), name
        # new == const counts (K5 over the new column's tile offsets), on its own and behind a selection
        o = t.ordinal
        assert dfdb_mod.nrow(v[ir.col(o("r_const")) == "missing", dfdb_mod.ALL]) == sum(x == b"missing" for x in want["r_const"]) == len(range(0, N, 7))
        assert dfdb_mod.nrow(v[ir.col(o("r_cat")) == "x", dfdb_mod.ALL]) == sum(x == b"x" for x in want["r_cat"])
        assert dfdb_mod.nrow(v[ir.coalesce(ir.col(o("r_null")) == "", False), dfdb_mod.ALL]) == sum(x == b"" for x in want["r_null"])
        assert np.array_equal(v[ir.coalesce(ir.ismissing(ir.col(o("r_null"))), False), dfdb_mod.ALL]._query().indices(),
                              np.array([i + 1 for i, x in enumerate(want["r_null"]) if x is None]))
        # sizeof sums
        assert dfdb_mod.sizeof(v.r_const).sum() == sum(len(x) for x in want["r_const"])
        assert dfdb_mod.sizeof(v.r_cat).sum() == sum(len(x) for x in want["r_cat"])
        # unique, in order of first appearance
        assert list(v.r_cat.unique()) == list(dict.fromkeys(strs(want["r_cat"])))
        assert list(v.r_null.unique()) == list(dict.fromkeys(strs(want["r_null"])))
        # a second coalesce over the new column
        check(dfdb_mod, t, coalesce_ref(want["r_null"], b"second"), v[dfdb_mod.ALL, project(dfdb_mod, t, "r_null", b"second")])
        check(dfdb_mod, t, coalesce_ref(data.cols["a_all"], want["r_null"]), v[dfdb_mod.ALL, project(dfdb_mod, t, "a_all", "r_null")])
        # a filtered view into another table
        s, m = selection_of(dfdb_mod, data, "predicate", t)
        t2.add_column_from("f", v[s, dfdb_mod.ALL][dfdb_mod.ALL, project(dfdb_mod, t, "a_every7th", "bn")])
        wf = expected(data, "a_every7th", "bn", m)
        ws, wd, _ = flat(wf)
        sizes, arena = dfdb_mod.DFView(t2)._query().materialize()[0]
        assert t2.getmeta("f").type == "Missing(String)" and np.array_equal(sizes, ws) and np.array_equal(arena, wd)
        assert list(dfdb_mod.DFView(t2).f.unique()) == list(dict.fromkeys(strs(wf)))
        # saved with the writer, read back by the oracle
        t2.add_column_from("g", dfdb_mod.coalesce(dfdb_mod.DFView(t2).f, ""))
        path = str(tmp_path / "tb")
        assert t2.save(path)["rows"] == int(m.sum())
        ot = oracle.Table.open(path)
        try:
            got = ot.view().materialize()
            assert np.array_equal(got[0][0], ws) and np.array_equal(got[0][1], wd)
            gs, gd, _ = flat(coalesce_ref(wf, b""))
            assert np.array_equal(got[1][0], gs) and np.array_equal(got[1][1], gd)
        finally:
            ot.close()
    finally:
        t2.close(); t.close()


# ---------------------------------------------------------------- out of core
def test_out_of_core_gives_the_same_answers(oracle, dfdb_mod, ctx, data, tmp_path):
    """the table written by the oracle's writer (String columns as Union{String,Missing}), opened with nothing resident in a context whose budget holds
    nothing: materialize and add_column_from stream it, two blocks per chunk"""
    from dfdb import ir
    names = ["a_every7th", "a_run-over-boundary", "a_all", "p", "bn", "bp"]
    ot = oracle.Table(block_size=1000)
    for n in names:
        ot.add_column(n, oracle.strings_to_flat(data.cols[n]), dtype=oracle.NULLABLE)
    ot.add_column("k", data.k)
    path = str(tmp_path / "ooc")
    ot.save(path)
    ot.close()
    c2 = dfdb_mod.Context()
    for key, val in (("hbm_budget_mb", 1), ("ooc_chunk_blocks", 2)):
        c2.set_option(key, val)
    lazy = dfdb_mod.open_table(path, load=False, ctx=c2)
    t2, t3 = dfdb_mod.DFTable.new(block_size=1000, ctx=c2), dfdb_mod.DFTable.new(block_size=1000, ctx=c2)
    try:
        v = dfdb_mod.DFView(lazy)
        m = data.k % 10 == 3
        for a, b in (("a_every7th", b"missing"), ("a_run-over-boundary", "bn"), ("a_all", b""), ("p", "bn"), ("a_every7th", "bp")):
            check(dfdb_mod, lazy, expected(data, a, b), v[dfdb_mod.ALL, project(dfdb_mod, lazy, a, b)])
            check(dfdb_mod, lazy, expected(data, a, b, m), v[ir.col(lazy.ordinal("k")) % 10 == 3, dfdb_mod.ALL][dfdb_mod.ALL, project(dfdb_mod, lazy, a, b)])
        check(dfdb_mod, lazy, [], v[ir.col(lazy.ordinal("k")) < 0, dfdb_mod.ALL][dfdb_mod.ALL, project(dfdb_mod, lazy, "a_every7th", b"missing")])
        assert not any(lazy.resident(i) for i in range(len(names) + 1))
        t2.add_column_from("r", dfdb_mod.coalesce(v.a_every7th, "missing"))
        t2.add_column_from("n", dfdb_mod.coalesce(v[dfdb_mod.ALL, "a_run-over-boundary"], v.bn))
        t3.add_column_from("f", v[ir.col(lazy.ordinal("k")) % 10 == 3, dfdb_mod.ALL][dfdb_mod.ALL, project(dfdb_mod, lazy, "a_run-over-boundary", "bn")])
        for tb, name, w in ((t2, "r", expected(data, "a_every7th", b"missing")), (t2, "n", expected(data, "a_run-over-boundary", "bn")),
                            (t3, "f", expected(data, "a_run-over-boundary", "bn", m))):
            ws, wd, _ = flat(w)
            sizes, arena = dfdb_mod.DFView(tb)[dfdb_mod.ALL, [name]]._query().materialize()[0]
            assert np.array_equal(sizes, ws) and np.array_equal(arena, wd), name
        assert t2.getmeta("r").type == "String" and t2.getmeta("n").type == "Missing(String)"
        assert dfdb_mod.nrow(dfdb_mod.DFView(t2)[ir.col(0) == "missing", dfdb_mod.ALL]) == len(range(0, N, 7))
        assert not any(lazy.resident(i) for i in range(len(names) + 1))
    finally:
        for tb in (t2, t3, lazy):
            tb.close()
        c2.close()


# ---------------------------------------------------------------- a wave that takes two tiles at a time
GATHER_PASSES = ("str_gather_sizes", "str_gather_bytes", "str_coalesce_sizes", "str_coalesce_bytes")


def launches(ctx, fn):
    """(what fn returns, launches per profile name of the K6 passes while it ran)"""
    ctx.profile(True)
    try:
        before = {k: ctx.profile_get(k)[0] for k in GATHER_PASSES}
        out = fn()
        return out, {k: ctx.profile_get(k)[0] - before[k] for k in GATHER_PASSES}
    finally:
        ctx.profile(False)


def test_two_tiles_per_wave_plain_and_coalesce(oracle, dfdb_mod, ctx):
    """From 16 384 tiles on, a wave of either K6 pass looks at `group` >= 2 tiles together (k_strings.hip gather_group).  16 386 tiles, the last one ragged:
    group is 2, the pairs are tiles (2m, 2m + 1).  The selection keeps rows in a few tiles only, so nearly every pair is empty and skipped: row 1; 200 rows
    over the boundary inside pair (2000, 2001), 100 per tile (more than one round of 64); 100 rows in tile 10001, whose partner 10000 is empty; the last
    1025 rows (a whole tile and the one-row ragged tile, which are a pair).  The columns are generated on the device."""
    from dfdb import ir
    n = 16384 * 1024 + 1025
    seed, seed2 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
    windows = [(0, 1), (2001 * 1024 - 100, 200), (10001 * 1024 + 300, 100), (n - 1025, 1025)]          # (first row, rows), rows counted from 0
    t = dfdb_mod.DFTable.new()
    try:
        t.add_generated("s", dfdb_mod.GEN_STR_BRANDS10, seed, n)
        t.add_generated("sm", dfdb_mod.GEN_STR_BRANDS10_MISSING, seed, n)
        t.add_generated("s2", dfdb_mod.GEN_STR_BRANDS10, seed2, n)
        t.add_generated("i", dfdb_mod.GEN_I64_IOTA, 0, n)                                               # i = the row number, from 1
        i, pred = ir.col(t.ordinal("i")), None
        for r0, k in windows:
            term = (i >= r0 + 1) & (i <= r0 + k)
            pred = term if pred is None else pred | term
        v = dfdb_mod.DFView(t)[pred, dfdb_mod.ALL]
        want_s = []
        for r0, k in windows:
            want_s += unflat(*oracle.gen_str(seed, r0, k))
        assert len(want_s) == sum(k for _, k in windows)

        q, ran = launches(ctx, lambda: check(dfdb_mod, t, want_s, v[dfdb_mod.ALL, ["s"]]))
        assert ran["str_gather_sizes"] >= 1 and ran["str_gather_bytes"] == 1 and ran["str_coalesce_sizes"] == 0 and ran["str_coalesce_bytes"] == 0, ran
        plain_s = q.materialize()[0]
        (sm_sizes, sm_arena), (s2_sizes, s2_arena) = v[dfdb_mod.ALL, ["sm", "s2"]]._query().materialize()
        got_sm, got_s2 = unflat(sm_sizes, sm_arena), unflat(s2_sizes, s2_arena)
        assert any(x is None for x in got_sm) and any(x is not None for x in got_sm)
        assert got_s2 == [x for r0, k in windows for x in unflat(*oracle.gen_str(seed2, r0, k))]

        q, ran = launches(ctx, lambda: check(dfdb_mod, t, want_s, v[dfdb_mod.ALL, project(dfdb_mod, t, "s", b"")]))     # a non-nullable a: the column itself
        assert ran["str_coalesce_sizes"] >= 1 and ran["str_coalesce_bytes"] == 1 and ran["str_gather_sizes"] == 0 and ran["str_gather_bytes"] == 0, ran
        got = q.materialize()[0]
        assert np.array_equal(got[0], plain_s[0]) and np.array_equal(got[1], plain_s[1])
        for b, second in (("s2", got_s2), (b"?", b"?")):
            _, ran = launches(ctx, lambda: check(dfdb_mod, t, coalesce_ref(got_sm, second), v[dfdb_mod.ALL, project(dfdb_mod, t, "sm", b)]))
            assert ran["str_coalesce_sizes"] >= 1 and ran["str_coalesce_bytes"] == 1 and ran["str_gather_sizes"] == 0 and ran["str_gather_bytes"] == 0, ran
    finally:
        t.close()
