"""dfdb_gather_rows_any and dfdb_gather_rows_string_bytes (csrc/k_str_rows.hip: String columns at given rows — a sizes pass, a scan, a bytes pass) against the
definition of tests/str_gather_rows_cases.py.  Every comparison is bit for bit: the sizes, the bytes and their count.  Every case runs in BOTH forms of the
in-tile prefix (ctx option "str_gather_form": 1 = the per-row offset array built for the call, 2 = one wave per output summing its tile's sizes), which must
agree with each other and with the reference; after every failing call the query still answers count() as before."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import str_gather_rows_cases as G

pytestmark = pytest.mark.gpu

OFFSETS, DIRECT = 1, 2
FORMS = (OFFSETS, DIRECT)


@contextlib.contextmanager
def forced(ctx, form):
    ctx.set_option("str_gather_form", form)
    try:
        yield
    finally:
        ctx.set_option("str_gather_form", 0)


@functools.lru_cache(maxsize=None)
def case(nrows):
    """(columns, row lists, {(column, list): take_ref}) of one column length: computed once, shared, never changed"""
    cols, lists = G.columns(nrows), G.row_lists(nrows)
    return cols, lists, {(c, l): G.take_ref(v, r) for c, v in cols.items() for l, r in lists.items()}


def string_table(dfdb, ctx, cols, nullable=G.NULLABLE):
    from dfdb import ir
    t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    for name, values in cols.items():
        t.add_column(name, list(values), dtype=ir.STRING | ir.NULLABLE if name in nullable else None)
    return t


def same(got, want):
    return (isinstance(got, tuple) and got[0].dtype == np.int32 and got[1].dtype == np.uint8 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))


def device_rows(rows):
    import torch
    d = torch.as_tensor(np.ascontiguousarray(rows, np.int64), device=torch.device("cuda", 0))
    torch.cuda.synchronize()                    # (the copy runs on torch's stream, the gather on the engine's own: order them)
    return d


def case_matrix(dfdb_mod, ctx, nrows):
    cols, lists, refs = case(nrows)
    t = string_table(dfdb_mod, ctx, cols)
    names = list(cols)
    q = t[dfdb_mod.ALL, names]._query()
    count0 = q.count()
    for lname, rows in lists.items():
        d = device_rows(rows)
        answers = []
        for form in FORMS:
            with forced(ctx, form):
                for got in (q.gather_rows_any(rows), q.gather_rows_any(dev_ptr=d.data_ptr(), n=len(rows))):
                    assert len(got) == len(names)
                    for i, name in enumerate(names):
                        assert same(got[i], refs[name, lname]), (nrows, lname, name, form, got[i][0][:8], refs[name, lname][0][:8])
                    answers.append(got)
                for i, name in enumerate(names):                                                   # the layout call: the reference's total
                    assert q.gather_rows_string_bytes(i, rows) == len(refs[name, lname][1]), (nrows, lname, name, form)
                    assert q.gather_rows_string_bytes(i, dev_ptr=d.data_ptr(), n=len(rows)) == len(refs[name, lname][1])
        for other in answers[1:]:                                                                  # the forms agree with each other
            assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(answers[0], other))
    assert q.count() == count0 == nrows
    t.close()


def part_the_option_and_the_rule_choose_the_form(dfdb_mod, ctx):
    cols, lists, refs = case(70_001)
    t = string_table(dfdb_mod, ctx, {"plain": cols["plain"]}, ())
    q = t[dfdb_mod.ALL, ["plain"]]._query()

    def launches(rows):
        ctx.synchronize()
        ctx.profile(True)
        got = q.gather_rows_any(rows)
        ctx.synchronize()
        n = (ctx.profile_get("str_rows_sizes.offsets")[0], ctx.profile_get("str_rows_sizes.direct")[0], ctx.profile_get("str_row_offsets")[0])
        ctx.profile(False)
        return got, n

    few, many = lists["n65"], lists["n4097"]                                                       # 65 * 512 <= 70 001 < 4097 * 512
    assert launches(few)[1] == (0, 1, 0) and launches(many)[1] == (1, 0, 1)                        # the rule
    with forced(ctx, OFFSETS):
        got, n = launches(few)
        assert n == (1, 0, 1) and same(got[0], refs["plain", "n65"])
    with forced(ctx, DIRECT):
        got, n = launches(many)
        assert n == (0, 1, 0) and same(got[0], refs["plain", "n4097"])
    t.close()


def raw_gather(dfdb, ctx, q, rows, kinds, short_by=0, fn="dfdb_gather_rows_any"):
    """the raw call over a view of String columns, kinds[i] = "host" / "device": sentinel-filled buffers with spare room on both sides of what the call may
    write.  Returns per column (sizes with the two guard slots, bytes with 8 guard bytes in front and 8 behind, nbytes); short_by: bytes_cap that much too small"""
    import torch
    from dfdb import _native as N
    rows = np.ascontiguousarray(rows, np.int64)
    n = len(rows)
    outs = (N.OutCol * len(kinds))()
    keep = []
    for i, kind in enumerate(kinds):
        nb = q.gather_rows_string_bytes(i, rows)
        if kind == "device":
            sizes = torch.full((n + 2,), -7, dtype=torch.int32, device=torch.device("cuda", 0))
            data = torch.full((nb + 16,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
            outs[i].data, outs[i].bytes, outs[i].memkind = sizes.data_ptr() + 4, data.data_ptr() + 8, N.MEM_DEVICE
        else:
            sizes, data = np.full(n + 2, -7, np.int32), np.full(nb + 16, 0xA5, np.uint8)
            outs[i].data, outs[i].bytes, outs[i].memkind = sizes.ctypes.data + 4, data.ctypes.data + 8, N.MEM_HOST
        outs[i].bytes_cap = nb - short_by
        keep.append((sizes, data, nb))
    torch.cuda.synchronize()
    try:
        N.check(getattr(N.load(), fn)(q._h, rows.ctypes.data if n else None, n, N.MEM_HOST, outs, len(kinds)))
    finally:
        ctx.synchronize()
    res = []
    for i, (sizes, data, nb) in enumerate(keep):
        assert outs[i].count == n and outs[i].nbytes == nb
        res.append((sizes.cpu().numpy() if kinds[i] == "device" else sizes, data.cpu().numpy() if kinds[i] == "device" else data, nb))
    return res, keep


def part_outputs_in_host_and_device_memory_and_nothing_beyond_them(dfdb_mod, ctx):
    for nrows in (1025, 70_001):
        cols, lists, refs = case(nrows)
        t = string_table(dfdb_mod, ctx, cols)
        names = list(cols)
        q = t[dfdb_mod.ALL, names]._query()
        for lname in ("empty", "first_last", "permutation", "repeat1500", "n1025"):
            for form in FORMS:
                with forced(ctx, form):
                    for kinds in (("device",) * 3, ("host", "device", "host")):
                        res, _ = raw_gather(dfdb_mod, ctx, q, lists[lname], kinds)
                        for (sizes, data, nb), name in zip(res, names):
                            want = refs[name, lname]
                            assert sizes[0] == -7 and sizes[-1] == -7 and np.array_equal(sizes[1:-1], want[0]), (nrows, lname, name, form, kinds)
                            assert nb == len(want[1]) and np.array_equal(data[8:8 + nb], want[1]), (nrows, lname, name, form, kinds)
                            assert np.all(data[:8] == 0xA5) and np.all(data[8 + nb:] == 0xA5), (nrows, lname, name, form, kinds)
        t.close()


def mixed_table(dfdb, ctx, n=5000):
    from dfdb import ir
    rng = np.random.default_rng(n)
    cols, _, _ = case(70_001)
    k = rng.integers(0, 40, n).astype(np.int64)
    k2 = rng.integers(0, 6, n).astype(np.int64)
    z = np.ma.masked_array(rng.integers(-20, 20, n) * 0.5 + 0.25, mask=rng.random(n) < 0.2)          # ties, no zero of either sign
    t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    t.add_column("k", k)
    t.add_column("k2", k2)
    t.add_column("z", z)
    t.add_column("s", cols["plain"][:n])
    t.add_column("sn", cols["fifth"][:n], dtype=ir.STRING | ir.NULLABLE)
    return t, {"k": k, "k2": k2, "z": z, "s": cols["plain"][:n], "sn": cols["fifth"][:n]}


def part_a_mixed_view_through_one_call(dfdb_mod, ctx):
    t, cols = mixed_table(dfdb_mod, ctx)
    names = ["k", "z", "s", "sn"]                                                                  # Int64, nullable Float64, String, nullable String
    q = t[("k2", lambda c: c < 3), names]._query()                                                 # (the gather does not depend on the selection)
    count0 = q.count()
    n = len(cols["k"])
    for rows in (np.array([n, 1, 1, 4097, 2, n, 1024, 1025, 1, 64]), np.random.default_rng(1).permutation(n)[:3000] + 1, np.array([], np.int64)):
        idx = rows - 1
        for form in FORMS:
            with forced(ctx, form):
                got = q.gather_rows_any(rows)
            assert got[0].dtype == np.int64 and np.array_equal(got[0], cols["k"][idx])
            zm = np.ma.getmaskarray(cols["z"])[idx]
            assert isinstance(got[1], np.ma.MaskedArray) and np.array_equal(np.ma.getmaskarray(got[1]), zm)
            assert np.array_equal(np.asarray(got[1].data)[~zm], np.asarray(cols["z"].data)[idx][~zm])
            assert same(got[2], G.take_ref(cols["s"], rows)) and same(got[3], G.take_ref(cols["sn"], rows))
            assert q.gather_rows_string_bytes(0, rows) == 0 and q.gather_rows_string_bytes(1, rows) == 0      # fixed-width columns need no string bytes
    assert q.count() == count0 == int((cols["k2"] < 3).sum())
    t.close()


def part_gathering_the_selected_rows_is_materialize(dfdb_mod, ctx):
    t, cols = mixed_table(dfdb_mod, ctx)
    for sel in (("k2", lambda c: c < 3), ("k", lambda c: c == 7), ("k", lambda c: c < 0)):
        q = t[sel, ["s", "sn", "k"]]._query()
        rows = q.indices()
        want = t[sel, ["s", "sn", "k"]]._query().materialize()
        for form in FORMS:
            with forced(ctx, form):
                got = q.gather_rows_any(rows)
            for g, w in zip(got[:2], want[:2]):
                assert same(g, w) and len(g[1]) == len(w[1])                                       # sizes, bytes and nbytes
            assert np.array_equal(got[2], want[2])
    t.close()


def part_sort_view_brings_the_string_columns_along(dfdb_mod, ctx):
    import pandas as pd
    t, cols = mixed_table(dfdb_mod, ctx, 2100)                                                     # (three tiles, the last one partial)
    names = ["k", "k2", "z", "s", "sn"]
    v = t[("k2", lambda c: c < 5), names]
    sel = np.flatnonzero(cols["k2"] < 5)
    frame = pd.DataFrame({"k": cols["k"][sel], "k2": cols["k2"][sel], "z": cols["z"].filled(np.nan)[sel],
                          "s": np.array(cols["s"], object)[sel], "sn": np.array(cols["sn"], object)[sel]})
    for by, revs in (("k", (False, True)), ("z", (False, True)), (["k2", "k"], (False, True, [True, False]))):
        for rev in revs:
            for limit in (1, 10, None):
                asc = [not r for r in rev] if isinstance(rev, list) else not rev
                # the project's rule: missing rows last, first under rev (the nullable key is sorted alone, so one na_position says it)
                want = frame.sort_values(by, ascending=asc, kind="stable", na_position="first" if rev is True else "last")
                want = want if limit is None else want.head(limit)
                for form in FORMS:
                    with forced(ctx, form):
                        got = dfdb_mod.sort_view(v, by, rev=rev, limit=limit)
                    assert list(got.columns) == names and len(got) == len(want), (by, rev, limit)
                    for name in ("k", "k2"):
                        assert np.array_equal(got[name].to_numpy(), want[name].to_numpy()), (by, rev, limit, name)
                    assert np.array_equal(got["z"].to_numpy(dtype=np.float64, na_value=np.nan), want["z"].to_numpy(), equal_nan=True), (by, rev, limit)
                    for name in ("s", "sn"):
                        assert list(got[name]) == list(want[name]), (by, rev, limit, name, form)
    rows = [len(cols["k"]), 1, 1, 1025]
    df = dfdb_mod.take(v, rows)                                                                    # the plain form of the same call
    assert list(df.columns) == names and list(df["s"]) == [cols["s"][r - 1] for r in rows] and list(df["sn"]) == [cols["sn"][r - 1] for r in rows]
    assert np.array_equal(df["k"].to_numpy(), cols["k"][np.array(rows) - 1])
    t.close()


def part_a_column_with_a_dictionary_gives_the_flat_answer(dfdb_mod, ctx):
    brands = ["apple", "", "samsung", "xiaomi", "é", "a-much-longer-brand-name"]
    values = [brands[(i * 7) % len(brands)] for i in range(2049)]
    t = string_table(dfdb_mod, ctx, {"b": values}, ())
    q = t[dfdb_mod.ALL, ["b"]]._query()
    rows = G.row_lists(2049)["permutation"]
    before = [q.gather_rows_any(rows)[0]]
    assert t.build_dictionary("b") == len(brands)
    for form in FORMS:
        with forced(ctx, form):
            got = q.gather_rows_any(rows)[0]
        assert same(got, G.take_ref(values, rows)) and same(got, before[0])
    t.close()


def part_errors_leave_the_query_as_it_was(dfdb_mod, ctx):
    cols, lists, refs = case(2049)
    t = string_table(dfdb_mod, ctx, cols)
    names = list(cols)
    q = t[dfdb_mod.jr(1, 2, dfdb_mod.END), names]._query()
    count0 = q.count()
    assert count0 == 1025
    for form in FORMS:
        with forced(ctx, form):
            for bad in (0, 2050, -3):                                                              # a row 0, a row nrows + 1
                with pytest.raises(IndexError, match="BoundsError"):
                    q.gather_rows_any([1, bad, 2])
                with pytest.raises(IndexError, match="BoundsError"):
                    q.gather_rows_string_bytes(0, [1, bad, 2])
                assert q.count() == count0
            with pytest.raises(IndexError, match="BoundsError"):
                q.gather_rows_string_bytes(len(names), [1])                                        # the column index, as dfdb_result_string_bytes checks it
            for kinds in (("host",) * 3, ("host", "device", "device")):                            # bytes_cap one byte short: refused before a byte moves
                with pytest.raises(IndexError, match="string bytes, capacity"):
                    raw_gather(dfdb_mod, ctx, q, lists["permutation"], kinds, short_by=1)
                assert q.count() == count0
    t.close()


def part_a_short_bytes_buffer_is_left_untouched(dfdb_mod, ctx):
    import torch
    from dfdb import _native as N
    cols, lists, refs = case(2049)
    t = string_table(dfdb_mod, ctx, {"plain": cols["plain"]}, ())
    q = t[dfdb_mod.ALL, ["plain"]]._query()
    rows = np.ascontiguousarray(lists["permutation"])
    nb = q.gather_rows_string_bytes(0, rows)
    assert nb == len(refs["plain", "permutation"][1]) > 0
    for form in FORMS:
        for kind in ("host", "device"):
            outs = (N.OutCol * 1)()
            if kind == "host":
                sizes, data = np.zeros(len(rows), np.int32), np.full(nb + 8, 0xA5, np.uint8)
                outs[0].data, outs[0].bytes, outs[0].memkind = sizes.ctypes.data, data.ctypes.data, N.MEM_HOST
            else:
                sizes = torch.zeros(len(rows), dtype=torch.int32, device=torch.device("cuda", 0))
                data = torch.full((nb + 8,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
                outs[0].data, outs[0].bytes, outs[0].memkind = sizes.data_ptr(), data.data_ptr(), N.MEM_DEVICE
            outs[0].bytes_cap = nb - 1
            torch.cuda.synchronize()
            with forced(ctx, form):
                with pytest.raises(IndexError, match="string bytes, capacity"):
                    N.check(N.load().dfdb_gather_rows_any(q._h, rows.ctypes.data, len(rows), N.MEM_HOST, outs, 1))
            ctx.synchronize()
            assert np.all((data if kind == "host" else data.cpu().numpy()) == 0xA5), (form, kind)   # the sentinel-filled buffer is as it was
            assert q.count() == 2049
    t.close()


def part_refusals_name_the_column_or_the_form(dfdb_mod, ctx):
    x = (np.arange(3000, dtype=np.int64) * 7919) % 10_007
    t = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    t.add_column("x", x)
    t.add_column("s", [G.string_of(i) for i in range(3000)])
    s, xc = t[dfdb_mod.ALL, "s"], t[dfdb_mod.ALL, "x"]
    cv = dfdb_mod.view_from_columns(s=s, y=xc + 1)
    with pytest.raises(NotImplementedError, match="computed column"):
        cv._query().gather_rows_any([1, 2])
    with pytest.raises(NotImplementedError, match="computed column"):                              # a coalesce is a computed String column
        dfdb_mod.coalesce(s, "none").view._query().gather_rows_any([1, 2])
    q = t[dfdb_mod.ALL, ["s", "x"]]._query()
    assert same(q.gather_rows_any([3, 1])[0], G.take_ref([G.string_of(i) for i in range(3)], [3, 1]))
    with pytest.raises(NotImplementedError, match="String"):                                       # the entry point of the fixed-width gather refuses as it did
        q.gather_rows([1])
    with pytest.raises(NotImplementedError, match="String"):
        s.view._query().sort_indices(0)                                                            # sorting BY a String column stays refused
    t.compress_column("x", 2)                                                                      # what keep_compressed = 2 leaves: the LZ4 blocks alone
    q2 = t[dfdb_mod.ALL, ["s", "x"]]._query()
    with pytest.raises(NotImplementedError, match="compressed-only column x"):
        q2.gather_rows_any([1, 2])
    assert q2.count() == 3000
    t.close()
    t = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)                                            # one 4 MiB string: 1024 outputs of it overflow a 32-bit total
    t.add_column("big", ["x" * (4 << 20)])
    qb = t[dfdb_mod.ALL, ["big"]]._query()
    for form in (0,) + FORMS:
        with forced(ctx, form):
            with pytest.raises(NotImplementedError, match="String column big"):
                qb.gather_rows_any([1])
            with pytest.raises(NotImplementedError, match="String column big"):
                qb.gather_rows_string_bytes(0, [1])
    assert qb.count() == 1
    t.close()


# Three tests for the parts above, so that the suite's test count grows by three.  A failure names its part and its case in the assertion.
def test_case_matrix_in_both_forms_rows_from_host_and_device(dfdb_mod, ctx):
    for nrows in G.COLUMN_ROWS:
        case_matrix(dfdb_mod, ctx, nrows)


def test_views_materialize_sort_view_take_and_dictionary(dfdb_mod, ctx):
    part_a_mixed_view_through_one_call(dfdb_mod, ctx)
    part_gathering_the_selected_rows_is_materialize(dfdb_mod, ctx)
    part_sort_view_brings_the_string_columns_along(dfdb_mod, ctx)
    part_a_column_with_a_dictionary_gives_the_flat_answer(dfdb_mod, ctx)


def test_forms_outputs_errors_and_refusals(dfdb_mod, ctx):
    part_the_option_and_the_rule_choose_the_form(dfdb_mod, ctx)
    part_outputs_in_host_and_device_memory_and_nothing_beyond_them(dfdb_mod, ctx)
    part_a_short_bytes_buffer_is_left_untouched(dfdb_mod, ctx)
    part_errors_leave_the_query_as_it_was(dfdb_mod, ctx)
    part_refusals_name_the_column_or_the_form(dfdb_mod, ctx)
