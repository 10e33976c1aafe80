"""datetime19(s) on the device: DFIR_CAST with the target DFDB_CAST_DATETIME over a String column (include/dfdb_ir.h).  The yardstick is
tests/datetime_reference.py, the Python restatement of the rule table (tests/test_datetime_cpu.py pins it); every comparison is bit-exact, every error is
checked by status (the exception class), message prefix and reported row.  The whole file runs with the conversion kernel and with the interpreter
(parse_kernel 1 / 0), the interpreter ahead of time and compiled at run time (jit 0 / 2)."""
import json
import os
import re

import numpy as np
import pytest

from datetime_reference import ARGUMENT, BOUNDS, RATA_DIE_MS, UNSUPPORTED, VALUE, datetime_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = 65536
EXC = {BOUNDS: IndexError, ARGUMENT: ValueError, UNSUPPORTED: NotImplementedError}          # statuses 5, 1 and 7
PREFIX = {BOUNDS: "BoundsError:", ARGUMENT: "ArgumentError: DateTime:", UNSUPPORTED: "parse: "}
SAMPLE = {BOUNDS: "2019-10-01 00:00", ARGUMENT: "2019-02-30 00:00:00 UTC", UNSUPPORTED: "2019-10-01 24:00:00 UTC"}
MODES = [(1, 0), (1, 2), (0, 0), (0, 2)]


@pytest.fixture(autouse=True, params=MODES, ids=["kernel-jit0", "kernel-jit2", "interp-jit0", "interp-jit2"])
def mode(ctx, request):
    """(parse_kernel, jit): a projected datetime19.(s) through k_str_datetime or through the interpreter's H_DATETIME, which runs ahead of time or compiled"""
    pk, jit = request.param
    ctx.set_option("parse_kernel", pk); ctx.set_option("jit", jit); ctx.set_option("jit_min_rows", 0)
    yield request.param
    ctx.set_option("parse_kernel", 1); ctx.set_option("jit", 1); ctx.set_option("jit_min_rows", 1 << 22)


def launches(ctx, fn):
    """(k_str_datetime launches, interpreter or compiled-interpreter projection launches) while fn runs"""
    names = ("str_datetime", "interp_project", "jit_project")
    ctx.profile(True)
    before = [ctx.profile_get(k)[0] for k in names]
    try:
        fn()
    finally:
        after = [ctx.profile_get(k)[0] for k in names]
        ctx.profile(False)
    return after[0] - before[0], after[1] - before[1] + after[2] - before[2]


def raises(kind, row):
    return pytest.raises(EXC[kind], match="^" + re.escape(PREFIX[kind]) + rf".*\(row {row}\)$")


def table_of(dfdb, strs, nullable=False, block_size=BS, ctx=None):
    from dfdb import ir
    t = dfdb.DFTable.new(block_size=block_size, ctx=ctx)
    t.add_column("s", list(strs), dtype=ir.STRING | (ir.NULLABLE if nullable else 0))
    t.add_column("k", np.arange(len(strs), dtype=np.int64))
    return t


def project_raw(dfdb, t, fn=None, sel=None):
    """the Int64 instants as the engine makes them (the query's own arrays: no conversion to datetime64 on the way)"""
    from dfdb import ir
    v = dfdb.DFView(t)
    if sel is not None:
        v = v[sel, dfdb.ALL]
    return v[dfdb.ALL, {"r": ("s", fn or ir.datetime19)}]._query().materialize()[0]


def expected(strs):
    out = []
    for s in strs:
        k, v = datetime_ref(s)
        assert k == VALUE, (s, k)
        out.append(v)
    return np.array(out, dtype=np.int64)


def same_bits(got, want):
    got = np.asarray(got)
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (int(bad[0]), got[bad[0]], want[bad[0]])


TAIL = " UTC+0:00"


def stamp(rng, length=23):
    """a valid row of `length` >= 19 bytes: random instant, random ignored bytes at the separators' places and behind byte 19"""
    y, mo, d = int(rng.integers(0, 10000)), int(rng.integers(1, 13)), int(rng.integers(1, 29))
    h, mi, s = int(rng.integers(0, 24)), int(rng.integers(0, 60)), int(rng.integers(0, 60))
    seps = "- :T/x" if rng.random() < 0.3 else None
    sp = [seps[int(rng.integers(0, len(seps)))] for _ in range(5)] if seps else ["-", "-", " ", ":", ":"]
    txt = f"{y:04d}{sp[0]}{mo:02d}{sp[1]}{d:02d}{sp[2]}{h:02d}{sp[3]}{mi:02d}{sp[4]}{s:02d}"
    return txt + (TAIL * 2)[: length - 19]


def mixed_rows(n, seed=1):
    rng = np.random.default_rng(seed)
    return [stamp(rng, int(rng.integers(19, 28))) for _ in range(n)]


# ---------------------------------------------------------------- typing
def test_result_type_logical_type_and_refusals(dfdb_mod, ctx):
    from dfdb import ir
    t = table_of(dfdb_mod, ["2019-10-01 00:00:00"] * 2)
    tn = table_of(dfdb_mod, ["2019-10-01 00:00:00", None], nullable=True)
    e = ir.datetime19(ir.col(0))
    for tb in (t, tn):
        assert tb.expr_dtype(e) == ir.I64                               # never Union{DateTime,Missing}: string(missing) is a string
        assert tb.expr_logical(e) == "DateTime"
        assert tb.expr_dtype(e >= np.datetime64("2019-10-02", "ms")) == ir.BOOL
        assert tb.expr_logical(e >= np.datetime64("2019-10-02", "ms")) == ""
        assert tb.expr_dtype(ir.div(e - 5, 86400000)) == ir.I64 and tb.expr_logical(ir.div(e - 5, 86400000)) == ""
    assert t.expr_logical(ir.col(1)) == "" and t.expr_logical(ir.col(0)) == ""
    for bad in (ir.cast(ir.col(1), ir.CAST_DATETIME),                    # a numeric operand
                ir.cast(ir.const("2019-10-01 00:00:00"), ir.CAST_DATETIME),   # a String operand that is no column leaf
                ir.cast(ir.col(0), 0x40 | ir.F64), ir.cast(ir.col(0), 0x40 | ir.I32), ir.cast(ir.col(1), 0x40 | ir.I8)):
        with pytest.raises(NotImplementedError, match="unsupported conversion"):
            t.expr_dtype(bad)
    assert t.expr_dtype(ir.parse(ir.I64, ir.col(0))) == ir.I64 and t.expr_logical(ir.parse(ir.I64, ir.col(0))) == ""    # parse is what it was


# ---------------------------------------------------------------- values
def test_known_answers_and_the_tutorials_first_rows(dfdb_mod, ctx):
    known = {"2019-10-01 00:00:11 UTC": 63705571211000, "1970-01-01 00:00:00": 62135683200000, "0000-01-01 00:00:00": -31536000000}
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "datetime_tutorial.json")))
    strs = list(known) + gold["strings"] + ["2019-10-01 00:00:00 UTC", "2019-10-01T00:00:00", "2019-10-01T00:00:00.123", "9999-12-31 23:59:59"]
    want = np.array(list(known.values()) + gold["instants_ms"] + [63705571200000] * 3 + [datetime_ref("9999-12-31 23:59:59")[1]], np.int64)
    same_bits(expected(strs), want)
    t = table_of(dfdb_mod, strs)
    same_bits(project_raw(dfdb_mod, t), want)
    got = dfdb_mod.materialize(dfdb_mod.datetime19(dfdb_mod.DFView(t).s))         # the front end's spelling: datetime64[ms] back
    assert got.dtype == np.dtype("datetime64[ms]")
    assert np.array_equal(got[3:13], np.array([s[:19] for s in gold["strings"]], dtype="datetime64[ms]"))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 37])
def test_row_counts_around_the_wave_and_the_tile(dfdb_mod, ctx, n):
    """lengths 19..27 mixed: a row starts on every byte alignment; the last count has a second wave in the workgroup, a partial last tile, a grid stride"""
    strs = mixed_rows(n, seed=n)
    if n >= 63:
        off = np.concatenate(([0], np.cumsum([len(s) for s in strs])[:-1]))
        assert set(int(o) % 8 for o in off[:1024]) == set(range(8))
    same_bits(project_raw(dfdb_mod, table_of(dfdb_mod, strs)), expected(strs))


def test_all_rows_23_bytes_wide(dfdb_mod, ctx):
    rng = np.random.default_rng(23)
    strs = [stamp(rng, 23) for _ in range(3 * 1024 + 5)]
    assert {len(s) for s in strs} == {23}
    same_bits(project_raw(dfdb_mod, table_of(dfdb_mod, strs)), expected(strs))


def test_a_tile_too_large_for_the_stage_equals_the_staged_path(dfdb_mod, ctx):
    rng = np.random.default_rng(40)
    short = [stamp(rng, 19) for _ in range(3 * 1024)]
    long = list(short)
    for i in range(1024, 2048):
        long[i] = short[i] + "." * 40                                   # 1024 rows x 59 bytes: more than the stage holds
    staged = project_raw(dfdb_mod, table_of(dfdb_mod, short))
    same_bits(staged, expected(short))
    same_bits(project_raw(dfdb_mod, table_of(dfdb_mod, long)), staged)
    long[1500] = "2019-10-01 00:61:00" + "." * 40
    with raises(ARGUMENT, 1500):
        project_raw(dfdb_mod, table_of(dfdb_mod, long))


DT_STAGE = 24576             # the bytes a wave stages for datetime19 (csrc/k_parse.hip: DatetimeConv::kStage)


def stage_edge_rows(rng, lead, tile1_bytes):
    """2048 rows, the two tiles of one workgroup: valid 23-byte rows, the second row of each tile with ignored bytes behind it up to the tile's byte total.
    Tile 0 holds the most bytes that are staged and leave tile 1 `lead` bytes above a 16-byte boundary; tile 1 holds tile1_bytes"""
    strs = []
    for total in (DT_STAGE - 16 - (16 - lead) % 16, tile1_bytes):
        rows = [stamp(rng, 23) for _ in range(1024)]
        assert total >= 23 * 1024
        rows[1] += "." * (total - 23 * 1024)
        strs += rows
    return strs


@pytest.mark.parametrize("mode", [(1, 0)], ids=["kernel"], indirect=True)
@pytest.mark.parametrize("lead", [0, 15])
def test_the_largest_staged_tile_and_the_smallest_direct_tile(dfdb_mod, ctx, mode, lead):
    """a tile `lead` bytes above a 16-byte boundary is staged exactly when its bytes + lead + 16 <= DT_STAGE: the tile that fills the stage to its last byte,
    and the same tile one byte longer, which is converted from the arena.  Both tiles belong to one workgroup, whose two stages are neighbours in LDS.  Then
    the same columns with an invalid row in each tile (the last row of tile 1 ends where the stage ends): values, error kind and error row"""
    from dfdb import ir
    staged = stage_edge_rows(np.random.default_rng(2300 + lead), lead, DT_STAGE - 16 - lead)
    direct = list(staged)
    direct[1025] += "."
    for strs, over in ((staged, 0), (direct, 1)):
        size = [len(s) for s in strs]
        assert len(size) == 2048 and set(size) - {size[1], size[1025]} == {23}
        assert sum(size[:1024]) % 16 == lead and sum(size[:1024]) + 16 <= DT_STAGE             # tile 0, at lead 0, is staged
        assert sum(size[1024:]) + lead + 16 == DT_STAGE + over
    want = expected(staged)
    same_bits(expected(direct), want)
    bad_rows = (700, 2047)
    good = np.ones(2048, bool)
    good[list(bad_rows)] = False
    got = []
    for strs in (staged, direct):
        t = table_of(dfdb_mod, strs)
        nk, ni = launches(ctx, lambda: got.append(project_raw(dfdb_mod, t)))
        assert nk >= 1 and ni == 0, (nk, ni)
        same_bits(got[-1], want)
        bad = list(strs)
        for r in bad_rows:
            bad[r] = strs[r][:5] + "13" + strs[r][7:]                     # month 13: the same bytes in all, an ArgumentError
            assert datetime_ref(bad[r])[0] == ARGUMENT and len(bad[r]) == len(strs[r])
        tb = table_of(dfdb_mod, bad)
        with raises(ARGUMENT, bad_rows[0]):
            project_raw(dfdb_mod, tb)
        with raises(ARGUMENT, bad_rows[1]):
            project_raw(dfdb_mod, tb, sel=ir.col(1) != bad_rows[0])
        same_bits(project_raw(dfdb_mod, tb, sel=(ir.col(1) != bad_rows[0]) & (ir.col(1) != bad_rows[1])), want[good])
    same_bits(got[0], got[1])


def test_selections_give_compacted_results_in_order(dfdb_mod, ctx):
    from dfdb import ir
    strs = mixed_rows(5 * 1024 + 100, seed=3)
    want = expected(strs)
    k = np.arange(len(strs))
    t = table_of(dfdb_mod, strs)
    same_bits(project_raw(dfdb_mod, t, sel=ir.col(1) % 3 == 0), want[k % 3 == 0])
    keep = (k >= 3 * 1024 + 7) & (k % 5 == 1)                             # whole tiles without a selected row in front
    same_bits(project_raw(dfdb_mod, t, sel=(ir.col(1) >= 3 * 1024 + 7) & (ir.col(1) % 5 == 1)), want[keep])
    same_bits(project_raw(dfdb_mod, t, sel=[2, 1025, 5000]), want[[1, 1024, 4999]])


def test_unselected_rows_are_not_evaluated(dfdb_mod, ctx):
    from dfdb import ir
    strs = mixed_rows(3000, seed=4)
    bad = {100: None, 1100: "2019-13-01 00:00:00", 2100: "short", 2500: "2019-10-01 24:00:00"}
    for r, v in bad.items():
        strs[r] = v
    t = table_of(dfdb_mod, strs, nullable=True)
    good = np.array([r not in bad for r in range(len(strs))])
    want = expected([s for s, g in zip(strs, good) if g])
    sel = (ir.col(1) != 100) & (ir.col(1) != 1100) & (ir.col(1) != 2100) & (ir.col(1) != 2500)
    same_bits(project_raw(dfdb_mod, t, sel=sel), want)
    with raises(ARGUMENT, 1100):                                          # one of them selected: that row is the error
        project_raw(dfdb_mod, t, sel=(ir.col(1) != 100) & (ir.col(1) != 2100) & (ir.col(1) != 2500))
    with raises(BOUNDS, 100):                                             # the missing row
        project_raw(dfdb_mod, t, sel=ir.col(1) >= 100)
    with raises(BOUNDS, 2100):
        project_raw(dfdb_mod, t, sel=ir.col(1) > 1100)


@pytest.mark.parametrize("bad", [None, "", "2019-10-01 00:00:0", "2019-10-01 00:00é", "2019-13-01 00:00:00", "2019-02-29 00:00:00", "1900-02-29 00:00:00",
                                 "2019-04-31 00:00:00", "2019-10-01 24:61:00", "2019-10-01 25:00:00", "2019-10-01 23:60:00", "2019-10-01 23:59:60",
                                 " 019-10-01 00:00:00", "2019é10-01 00:00:00", b"2019-10\xff01 00:00:00", "2019-1a-01 00:00:00"])
def test_each_rule_raises_with_its_row(dfdb_mod, ctx, bad):
    """a projection, a larger expression, a predicate and add_column: status, prefix and row"""
    from dfdb import ir
    kind = datetime_ref(bad)[0]
    assert kind != VALUE
    row = 1024 + 333
    strs = mixed_rows(2 * 1024 + 10, seed=6)
    strs[row] = bad
    t = table_of(dfdb_mod, strs, nullable=True)
    with raises(kind, row):
        project_raw(dfdb_mod, t)
    with raises(kind, row):
        project_raw(dfdb_mod, t, fn=lambda s: ir.datetime19(s) + 1)
    with raises(kind, row):
        dfdb_mod.DFView(t)[ir.datetime19(ir.col(0)) >= 0, dfdb_mod.ALL]._query().indices()
    t2 = table_of(dfdb_mod, ["x"] * len(strs))
    with raises(kind, row):
        t2.add_column("dt", dfdb_mod.datetime19(dfdb_mod.DFView(t).s))
    assert len(t2.columns_meta()) == 2


def test_valid_neighbours_of_the_rules_are_values(dfdb_mod, ctx):
    strs = ["2020-02-29 00:00:00", "2000-02-29 23:59:59", "0000-02-29 00:00:00", "2019-10-01 00:00:00é", b"2019-10-01 00:00:00\xff\xfe", "2019x10y01z00w00v00",
            "2019-12-31 23:59:59 and then some text that is ignored", "2019-10-01 00:00:00"]
    same_bits(project_raw(dfdb_mod, table_of(dfdb_mod, strs)), expected(strs))


@pytest.mark.parametrize("first,second", [(BOUNDS, ARGUMENT), (ARGUMENT, UNSUPPORTED), (UNSUPPORTED, BOUNDS)])
@pytest.mark.parametrize("rows", [(700, 1024 + 5), (1024 + 5, 1024 + 900)], ids=["two-tiles", "one-tile"])
def test_the_smaller_row_decides_between_two_kinds(dfdb_mod, ctx, first, second, rows):
    from dfdb import ir
    strs = mixed_rows(3 * 1024, seed=7)
    strs[rows[0]], strs[rows[1]] = SAMPLE[first], SAMPLE[second]
    t = table_of(dfdb_mod, strs)
    with raises(first, rows[0]):
        project_raw(dfdb_mod, t)
    with raises(first, rows[0]):
        dfdb_mod.DFView(t)[ir.datetime19(ir.col(0)) > 5, dfdb_mod.ALL]._query().indices()
    with raises(second, rows[1]):                                        # the first one unselected: the second is the smallest
        project_raw(dfdb_mod, t, sel=ir.col(1) != rows[0])


# ---------------------------------------------------------------- routing
@pytest.fixture(scope="module")
def ascending(dfdb_mod, ctx):
    """the tutorial's column: 23-byte strings ascending by seconds from 2019-10-01, in a Union{String,Missing} column without missing rows"""
    n = 4 * 1024 + 321
    base = np.datetime64("2019-10-01T00:00:00", "s")
    inst = base + (np.arange(n) * 61).astype("timedelta64[s]")
    strs = [str(x).replace("T", " ") + " UTC" for x in inst]
    assert len(strs[0]) == 23 and strs[0] == "2019-10-01 00:00:00 UTC"
    return table_of(dfdb_mod, strs, nullable=True), strs, inst.astype("datetime64[ms]")


def test_the_plain_cast_runs_where_the_knob_says(dfdb_mod, ctx, mode, ascending):
    t, strs, inst = ascending
    want = inst.astype(np.int64) + RATA_DIE_MS
    same_bits(want, expected(strs))
    out = {}
    nk, ni = launches(ctx, lambda: out.__setitem__("r", project_raw(dfdb_mod, t)))
    assert (nk >= 1 and ni == 0) if mode[0] else (nk == 0 and ni >= 1), (mode, nk, ni)
    same_bits(out["r"], want)


def test_the_cast_as_a_predicate_operand_and_inside_a_larger_expression(dfdb_mod, ctx, mode, ascending):
    from dfdb import ir
    t, strs, inst = ascending
    cut = np.datetime64("2019-10-02T00:00:00", "ms")
    v = dfdb_mod.DFView(t)[ir.datetime19(ir.col(0)) >= cut, dfdb_mod.ALL]
    assert dfdb_mod.nrow(v) == int((inst >= cut).sum()) > 0
    assert np.array_equal(v._query().indices(), np.nonzero(inst >= cut)[0] + 1)
    c = int(cut.astype(np.int64)) + RATA_DIE_MS
    out = {}
    nk, ni = launches(ctx, lambda: out.__setitem__("r", project_raw(dfdb_mod, t, fn=lambda s: ir.div(ir.datetime19(s) - c, 86400000))))
    assert nk == 0 and ni >= 1, (nk, ni)                                 # not the plain cast: the interpreter, whatever the knob says
    want = inst.astype(np.int64) + RATA_DIE_MS - c
    same_bits(out["r"], (np.sign(want) * (np.abs(want) // 86400000)).astype(np.int64))      # Julia's ÷ truncates


# ---------------------------------------------------------------- a DateTime column
def test_add_column_makes_a_datetime_column_that_survives_the_writer(dfdb_mod, ctx, ascending, tmp_path):
    t, strs, inst = ascending
    t2 = table_of(dfdb_mod, strs)
    t2.add_column("dt", dfdb_mod.datetime19(dfdb_mod.DFView(t).s))
    assert t2.getmeta("dt").type == "DateTime" and t2.getmeta("dt").logical == "DateTime"
    got = dfdb_mod.materialize(dfdb_mod.DFView(t2)[dfdb_mod.ALL, ["dt"]])["dt"].to_numpy()
    want = np.array([s[:19] for s in strs], dtype="datetime64[ms]")
    assert np.array_equal(got.astype("datetime64[ms]"), want) and np.array_equal(want, inst)
    t2.add_column("dt2", dfdb_mod.DFView(t2)[dfdb_mod.ALL, {"r": ("s", dfdb_mod.ir.datetime19)}])          # a one-column view, into the view's own table
    assert t2.getmeta("dt2").type == "DateTime"
    path = str(tmp_path / "tb")
    assert t2.save(path)["rows"] == len(strs)
    t3 = dfdb_mod.open_table(path)
    try:
        assert t3.getmeta("dt").type == "DateTime" and t3.getmeta("dt2").type == "DateTime"
        back = dfdb_mod.materialize(dfdb_mod.DFView(t3)[dfdb_mod.ALL, ["dt"]])["dt"].to_numpy()
        assert np.array_equal(back.astype("datetime64[ms]"), want)
        same_bits(dfdb_mod.DFView(t3)[dfdb_mod.ALL, ["dt2"]]._query().materialize()[0], want.astype(np.int64) + RATA_DIE_MS)
    finally:
        t3.close()


def test_out_of_core_gives_the_same_column_and_global_rows(dfdb_mod, ctx, mode, tmp_path):
    """a context whose budget holds nothing, blocks of 100 rows, two blocks per chunk"""
    from dfdb import ir
    n, row = 437, 312
    strs = mixed_rows(n, seed=9)
    want = expected(strs)
    bad = list(strs)
    bad[row], bad[row + 50] = SAMPLE[BOUNDS], SAMPLE[ARGUMENT]
    for name, col in (("good", strs), ("bad", bad)):
        tb = table_of(dfdb_mod, col, nullable=True, block_size=100)
        tb.save(str(tmp_path / name))
        tb.close()
    c2 = dfdb_mod.Context()
    for k, v in (("hbm_budget_mb", 1), ("ooc_chunk_blocks", 2), ("parse_kernel", mode[0]), ("jit", mode[1]), ("jit_min_rows", 0)):
        c2.set_option(k, v)
    lazy = dfdb_mod.open_table(str(tmp_path / "good"), load=False, ctx=c2)
    lazy_bad = dfdb_mod.open_table(str(tmp_path / "bad"), load=False, ctx=c2)
    t2, t4 = dfdb_mod.DFTable.new(block_size=100, ctx=c2), dfdb_mod.DFTable.new(block_size=100, ctx=c2)
    try:
        same_bits(project_raw(dfdb_mod, lazy), want)
        same_bits(project_raw(dfdb_mod, lazy, sel=ir.col(1) % 3 == 0), want[np.arange(n) % 3 == 0])
        got = dfdb_mod.materialize(dfdb_mod.datetime19(dfdb_mod.DFView(lazy).s))
        assert got.dtype == np.dtype("datetime64[ms]") and np.array_equal(got.astype(np.int64) + RATA_DIE_MS, want)
        t2.add_column("dt", dfdb_mod.datetime19(dfdb_mod.DFView(lazy).s))
        assert t2.getmeta("dt").type == "DateTime"
        same_bits(dfdb_mod.DFView(t2)._query().materialize()[0], want)
        assert not lazy.resident(0)
        with raises(BOUNDS, row):
            project_raw(dfdb_mod, lazy_bad)
        with raises(BOUNDS, row):
            dfdb_mod.DFView(lazy_bad)[ir.datetime19(ir.col(0)) > 0, dfdb_mod.ALL]._query().count()
        with raises(ARGUMENT, row + 50):
            project_raw(dfdb_mod, lazy_bad, sel=ir.col(1) != row)
        with raises(BOUNDS, row):
            t4.add_column("dt", dfdb_mod.datetime19(dfdb_mod.DFView(lazy_bad).s))
    finally:
        # every table of the context is closed before the context: a query that outlives its table is orphaned by the close (one caught in the traceback of a
        # raised error is freed by a later garbage collection), and one that outlived its context would reach through a table into freed memory
        for tb in (t2, t4, lazy, lazy_bad):
            tb.close()
        c2.close()


def test_three_shards_agree_on_the_smallest_row_and_its_kind(dfdb_mod, ctx, mode, tmp_path):
    from dfdb import group as G, _native as NAT, ir
    bs, n = 128, 9 * 128 + 17                                            # 10 blocks: shards of 4 / 4 / 2
    rows = (300, 4 * bs + 77, 9 * bs + 5)
    strs = mixed_rows(n, seed=10)
    want = expected(strs)
    cases = {"good": {}, "b20": {rows[2]: SAMPLE[BOUNDS], rows[0]: SAMPLE[ARGUMENT]}, "b12": {rows[1]: SAMPLE[UNSUPPORTED], rows[2]: SAMPLE[ARGUMENT]},
             "b2": {rows[2]: SAMPLE[BOUNDS]}}
    for name, bad in cases.items():
        col = list(strs)
        for r, v in bad.items():
            col[r] = v
        tb = table_of(dfdb_mod, col, nullable=True, block_size=bs)
        tb.save(str(tmp_path / name))
        tb.close()
    g = G.Group.create([0, 0, 0], NAT.EXCHANGE_HOST)
    try:
        for k, v in (("parse_kernel", mode[0]), ("jit", mode[1]), ("jit_min_rows", 0)):
            g.set_option(k, v)
        proj = {"r": ("s", ir.datetime19)}
        gt = G.GroupTable.open(g, str(tmp_path / "good"))
        assert [gt.shard(l).view()._query().count() for l in range(3)] == [4 * bs, 4 * bs, n - 8 * bs]
        same_bits(G._gq(gt.view()[dfdb_mod.ALL, proj]).materialize()[0], want)
        same_bits(G._gq(gt.view()[ir.col(1) % 3 == 0, dfdb_mod.ALL][dfdb_mod.ALL, proj]).materialize()[0], want[np.arange(n) % 3 == 0])
        cut = int(np.median(want))
        assert G.gnrow(gt.view()[ir.datetime19(ir.col(0)) >= cut, dfdb_mod.ALL]) == int((want >= cut).sum())
        gt.close()
        for name, kind, row in (("b20", ARGUMENT, rows[0]), ("b12", UNSUPPORTED, rows[1]), ("b2", BOUNDS, rows[2])):
            gt = G.GroupTable.open(g, str(tmp_path / name))
            with raises(kind, row):
                G._gq(gt.view()[dfdb_mod.ALL, proj]).materialize()
            with raises(kind, row):
                G.gnrow(gt.view()[ir.datetime19(ir.col(0)) > 0, dfdb_mod.ALL])
            with raises(kind, row):
                G.gindices(gt.view()[ir.datetime19(ir.col(0)) > 0, dfdb_mod.ALL])
            assert G.gnrow(gt.view()[ir.col(1) % 2 == 0, dfdb_mod.ALL]) == (n + 1) // 2      # the group is fine afterwards
            gt.close()
    finally:
        g.close()


# ---------------------------------------------------------------- differential fuzz
def fuzz_rows(n, seed):
    """(rows, labels): lengths, separators, digits and damage drawn so that every rule occurs; the label names the rule the generator aimed at"""
    rng = np.random.default_rng(seed)
    rows, labels = [], []
    for _ in range(n):
        s = stamp(rng, int(rng.integers(19, 28)))
        r = rng.random()
        label = "value"
        if r < 0.004:
            s, label = None, "missing"
        elif r < 0.008:
            s, label = s[: int(rng.integers(0, 19))], "short"
        elif r < 0.012:
            cut = int(rng.integers(1, 17))
            s, label = s[:cut] + "é", "short-nonascii"
        elif r < 0.016:
            p = int(rng.integers(0, 19))
            s, label = s.encode()[:p] + b"\xc3" + s.encode()[p + 1:], "nonascii"
        elif r < 0.020:
            p = int(rng.choice([0, 1, 2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 17, 18]))
            s, label = s[:p] + " +-a:/"[int(rng.integers(0, 6))] + s[p + 1:], "nondigit"
        elif r < 0.024:
            s, label = s[:5] + ("00", "13", "99")[int(rng.integers(0, 3))] + s[7:], "month"
        elif r < 0.028:
            s, label = s[:5] + ("02-30", "04-31", "01-00", "12-32", "02-29")[int(rng.integers(0, 5))] + s[10:], "day"
        elif r < 0.032:
            s, label = s[:11] + ("25", "99", "60")[int(rng.integers(0, 3))] + s[13:], "hour"
        elif r < 0.036:
            s, label = s[:11] + "24" + s[13:14] + ("00", "61")[int(rng.integers(0, 2))] + s[16:], "hour24"
        elif r < 0.040:
            s, label = s[:14] + ("60", "99")[int(rng.integers(0, 2))] + s[16:], "minute"
        elif r < 0.044:
            s, label = s[:17] + ("60", "75")[int(rng.integers(0, 2))] + s[19:], "second"
        elif r < 0.050:
            s, label = s[:19] + "é\xff", "tail-nonascii"
        rows.append(s); labels.append(label)
    return rows, labels


@pytest.fixture(scope="module")
def fuzz(dfdb_mod, ctx):
    rows, labels = fuzz_rows(20_000, seed=2019)
    ref = [datetime_ref(s) for s in rows]
    t = table_of(dfdb_mod, rows, nullable=True)
    return t, rows, labels, ref


def test_differential_fuzz(dfdb_mod, ctx, fuzz):
    t, rows, labels, ref = fuzz
    # the generated data holds every rule, by the reference alone
    aimed = {"missing": {BOUNDS}, "short": {BOUNDS}, "short-nonascii": {UNSUPPORTED}, "nonascii": {UNSUPPORTED}, "nondigit": {UNSUPPORTED}, "month": {ARGUMENT},
             "hour": {ARGUMENT}, "hour24": {UNSUPPORTED}, "minute": {ARGUMENT}, "second": {ARGUMENT}, "tail-nonascii": {VALUE}, "value": {VALUE}}
    seen = {}
    for lb, (kd, _) in zip(labels, ref):
        seen.setdefault(lb, set()).add(kd)
    for lb, kinds in aimed.items():
        assert seen.get(lb) == kinds, (lb, seen.get(lb))
    assert seen["day"] == {ARGUMENT, VALUE}                               # 02-29 is a day of the leap years
    assert {len(s) % 8 for s in rows if isinstance(s, str)} == set(range(8))
    alive = np.ones(len(rows), bool)
    for _ in range(8):
        bad = [i for i in np.nonzero(alive)[0] if ref[i][0] != VALUE]
        if not bad:
            break
        sel = (np.nonzero(alive)[0] + 1).tolist()
        with raises(ref[bad[0]][0], bad[0]):
            project_raw(dfdb_mod, t, sel=sel)
        alive[bad[0]] = False                                            # drop that row and ask again: a wrong first answer cannot hide behind later ones
    good = np.array([kd == VALUE for kd, _ in ref])
    assert good.sum() > 18_000 and (~good).sum() > 500
    same_bits(project_raw(dfdb_mod, t, sel=(np.nonzero(good)[0] + 1).tolist()), np.array([v for kd, v in ref if kd == VALUE], np.int64))
