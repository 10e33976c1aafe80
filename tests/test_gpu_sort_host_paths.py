"""What the host side of csrc/sort.cpp launches, pinned: the sort driver (one key, a top-k cut, a nullable key, two keys) and the row gather (dfdb_gather_rows
and dfdb_gather_rows_any over the same fixed-width view) each counted per call with the context's profile.  The counts are LaunchTimer scopes, so the two
scans of a count phase are one "scan_counts"; they follow from the code: a build or a rekey that has to count first (a nullable key, a cut) runs twice and
scans once more, every digit pass is one count, one scan and one scatter, every key after the most minor one lays one order.  The answers of the counted
calls are compared too, with tests/sort_cases.py and tests/sort_multi_cases.py and with the columns themselves."""
import numpy as np
import pytest

import order_stat_cases as K
import sort_cases as S
import sort_multi_cases as M

pytestmark = pytest.mark.gpu

NROWS = 5000                                                # two 4096-pair chunks, five 1024-row tiles
SORT_NAMES = ("sort_build", "sort_rekey", "sort_order", "scan_counts", "sort_count", "sort_scatter", "sort_emit")
GATHER_NAMES = ("gather_rows", "str_rows_sizes", "str_row_offsets", "str_rows_bytes")


def table_of(dfdb, ctx, cols):
    """name -> values or (values, missing flags), the bytes under a flag left as they are"""
    from dfdb import _native as N, ir
    t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    for name, v in cols.items():
        arr, m = (np.ascontiguousarray(v[0]), np.ascontiguousarray(v[1], np.uint8)) if isinstance(v, tuple) else (np.ascontiguousarray(v), None)
        N.check(N.load().dfdb_table_add_column(t._h, name.encode(), ir.dtype_of_numpy(arr.dtype) | (ir.NULLABLE if m is not None else 0), len(arr), arr.ctypes.data, None, 0,
                                               m.ctypes.data if m is not None else None))
    return t


def counted(ctx, names, call):
    """(what call() returns, {name: scopes counted while it ran})"""
    ctx.synchronize()
    ctx.profile(True)
    try:
        got = call()
        ctx.synchronize()
        return got, {k: ctx.profile_get(k)[0] for k in names}
    finally:
        ctx.profile(False)


def sort_counts(first_counts, later_nullable, passes):
    """first_counts: the most minor key's build counts before it places (a nullable key, a cut); later_nullable: one flag per further key"""
    return {"sort_build": 2 if first_counts else 1, "sort_rekey": sum(2 if nl else 1 for nl in later_nullable), "sort_order": len(later_nullable),
            "scan_counts": passes + int(first_counts) + sum(map(int, later_nullable)), "sort_count": passes, "sort_scatter": passes, "sort_emit": 1}


def part_one_key_launches(dfdb_mod, ctx, t, x, miss):
    for name, limit, first_counts in (("plain", None, False), ("plain", 10, True), ("nullable", None, True)):
        m = miss if name == "nullable" else None
        q = t[dfdb_mod.ALL, name].view._query()
        assert q.count() == NROWS
        (rows, info), n = counted(ctx, SORT_NAMES, lambda: q.sort_indices(0, False, limit))
        assert np.array_equal(rows, S.sortperm_ref(x, m, None, False, limit)), (name, limit)
        assert info[0] == NROWS and info[1] == S.candidates_ref(x, m, None, False, limit) and (info[2], info[3]) == S.passes_ref(x, m, None, False, limit), (name, limit, info)
        assert info[2] == (1 if limit else 2), (name, limit, info)                  # 0 .. 599: two key bytes vary; the 18 pairs the cut keeps: one
        assert n == sort_counts(first_counts, (), info[2]), (name, limit, info, n)


def part_two_key_launches(dfdb_mod, ctx, t, x, miss):
    for keys in (("nullable", "plain"), ("plain", "nullable")):
        missings = [miss if k == "nullable" else None for k in keys]
        q = t[dfdb_mod.ALL, list(keys)]._query()
        assert q.count() == NROWS
        (rows, info), n = counted(ctx, SORT_NAMES, lambda: q.sort_indices_n([0, 1], [False, True]))
        assert np.array_equal(rows, M.sortperm_multi_ref([x, x], missings, None, [False, True])), keys
        assert info == M.info_multi_ref([x, x], missings) and info[2] == 4, (keys, info)
        assert n == sort_counts(keys[1] == "nullable", (keys[0] == "nullable",), info[2]), (keys, info, n)


# ---------------------------------------------------------------- the row gather: both entry points over one fixed-width view
def row_list(n):
    """1-based rows: a descending run from the last row, a row five times over, then any rows"""
    rng = np.random.default_rng([n, 5])
    return np.concatenate([np.arange(NROWS, NROWS - 40, -1), np.full(5, 17), rng.integers(1, NROWS + 1, n)])[:n].astype(np.int64)


def same_columns(got, cols, rows):
    for g, v in zip(got, cols.values()):
        want, wm = (v[0][rows - 1], np.asarray(v[1], bool)[rows - 1]) if isinstance(v, tuple) else (v[rows - 1], None)
        assert (wm is None) != isinstance(g, np.ma.MaskedArray) and g.dtype == want.dtype
        if wm is not None:
            assert np.array_equal(np.ma.getmaskarray(g), wm)
        assert np.array_equal(K.bits_of(np.ma.getdata(g)), K.bits_of(want))


def part_gather_launches(ctx, q, cols):
    import torch
    for n in (1, 1024, 1025):
        rows = row_list(n)
        d = torch.as_tensor(rows, device=torch.device("cuda", 0))
        torch.cuda.synchronize()                # (the copy runs on torch's stream, the gather on the engine's own: order them)
        for where, args in (("host", dict(rows=rows)), ("device", dict(dev_ptr=d.data_ptr(), n=n))):
            for call in (q.gather_rows, q.gather_rows_any):
                got, cnt = counted(ctx, GATHER_NAMES, lambda: call(**args))
                same_columns(got, cols, rows)
                assert cnt == {"gather_rows": len(cols), "str_rows_sizes": 0, "str_row_offsets": 0, "str_rows_bytes": 0}, (call.__name__, n, where, cnt)


def part_gather_refuses_a_row_outside_and_goes_on(q, cols):
    rows = row_list(65)
    for call in (q.gather_rows, q.gather_rows_any):
        with pytest.raises(IndexError, match="BoundsError"):
            call([NROWS + 1])
        same_columns(call(rows), cols, rows)


def test_sort_and_gather_launch_what_they_launched(dfdb_mod, ctx):
    x = (np.arange(NROWS) % 600).astype(np.int64)
    miss = np.arange(NROWS) % 7 == 6
    t = table_of(dfdb_mod, ctx, {"plain": x, "nullable": (x, miss)})
    part_one_key_launches(dfdb_mod, ctx, t, x, miss)
    part_two_key_launches(dfdb_mod, ctx, t, x, miss)
    t.close()
    rng = np.random.default_rng(NROWS)
    cols = {"i": rng.integers(-1000, 1000, NROWS).astype(np.int32), "f": (rng.standard_normal(NROWS), np.arange(NROWS) % 5 == 2),
            "u": rng.integers(0, 256, NROWS).astype(np.uint8)}
    t = table_of(dfdb_mod, ctx, cols)
    q = t[dfdb_mod.ALL, list(cols)]._query()
    part_gather_launches(ctx, q, cols)
    part_gather_refuses_a_row_outside_and_goes_on(q, cols)
    t.close()

