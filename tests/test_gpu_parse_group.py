"""parse(T, s) over block-range shards (csrc/group.cpp): values, and above all errors — which exception, with which table row, on every rank.

A parse error carries its row and one of four reasons; between ranks it travels as the fault key `(row + 1) << 8 | reason << 4 | status`, and a rank that does
not own the failing shard rebuilds the exception from the key alone (settle_fault).  One process with three shards on device 0 checks the values and the
agreed error of every entry point against the single table; three processes over gloo check the rebuilt error on the ranks that do not own the bad row.
The yardstick is tests/parse_reference.py, as in test_gpu_parse.py."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import parse_reference as R
from parse_reference import ARGUMENT, METHOD, OVERFLOW, UNSUPPORTED, parse_ref
from test_gpu_group import _free_port
from test_gpu_parse import ERRORS, EXC, PREFIX, expected, messy_strings, raises, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS, WORLD = 4096, 3
N = 9 * BS + 123                                            # 10 blocks, the last one ragged: shards of 4 / 4 / 2 blocks
ROWS = (1500, 4 * BS + 777, 9 * BS + 50)                    # one row in each shard's block range; the last in the ragged block
SAMPLE = {}
for _bad, _kind in ERRORS:
    SAMPLE.setdefault(_kind, _bad)
KINDS = (ARGUMENT, OVERFLOW, METHOD, UNSUPPORTED)
KIND_ID = {ARGUMENT: "argument", OVERFLOW: "overflow", METHOD: "method", UNSUPPORTED: "unsupported"}


def shard_of(row):
    from dfdb import sharding
    for r in range(WORLD):
        b0, b1 = sharding.block_range(-(-N // BS), r, WORLD)
        if b0 * BS <= row < b1 * BS:
            return r
    raise AssertionError(row)


def base_columns():
    rng = np.random.default_rng(7)
    vals = rng.integers(-10**12, 10**12, N).astype(np.int64)
    vals[::97] = rng.integers(2**62, 2**63 - 1, len(vals[::97]))             # 19 digits
    s = [str(int(v)) for v in vals]
    s8 = [str(int(v) % 256) for v in vals]
    sf = ["%d.%02d" % (int(v) % 100_000, (int(v) // 7) % 100) for v in vals]
    return vals, {"s": s, "k": np.arange(N, dtype=np.int64), "z": np.ones(N, np.int64), "s8": s8, "sf": sf}


def write_table(oracle, path, cols):
    """the oracle's writer; the String columns are Union{String,Missing} whether or not a row is missing"""
    ot = oracle.Table(block_size=BS)
    for k, v in cols.items():
        if isinstance(v, list):
            ot.add_column(k, oracle.strings_to_flat(v), dtype=oracle.NULLABLE)
        else:
            ot.add_column(k, v)
    ot.save(path)
    ot.close()


@pytest.fixture(scope="module")
def group(dfdb_mod, ctx):
    from dfdb import group as G, _native as NAT
    g = G.Group.create([0] * WORLD, NAT.EXCHANGE_HOST)
    yield g
    g.close()


@pytest.fixture(scope="module")
def tables(oracle, dfdb_mod, ctx, group, tmp_path_factory):
    """get(bad rows {row: string}, zero divisors [rows]) -> (group table, single table, the s column): written once per shape, opened both ways"""
    from dfdb import group as G
    vals, base = base_columns()
    root = tmp_path_factory.mktemp("parse_group")
    made = {}

    def get(bad=None, zeros=()):
        key = (tuple(sorted((bad or {}).items(), key=lambda kv: kv[0])), tuple(zeros))
        if key not in made:
            cols = dict(base)
            cols["s"] = list(base["s"])
            for row, v in (bad or {}).items():
                cols["s"][row] = v
            if zeros:
                cols["z"] = base["z"].copy()
                cols["z"][list(zeros)] = 0
            path = str(root / ("t%d" % len(made)))
            write_table(oracle, path, cols)
            gt = G.GroupTable.open(group, path)
            assert gt.nrows == N and [gt.shard(l).view()._query().count() for l in range(WORLD)] == [4 * BS, 4 * BS, N - 8 * BS]
            made[key] = (gt, dfdb_mod.open_table(path, ctx=ctx), cols["s"])
        return made[key]
    get.vals, get.base = vals, base
    yield get
    for gt, t1, _ in made.values():
        gt.close(); t1.close()


@pytest.fixture(params=[(0, 1), (0, 0), (2, 1), (2, 0)], ids=["jit0-kernel", "jit0-interp", "jit2-kernel", "jit2-interp"])
def mode(ctx, group, request):
    """the interpreter ahead of time and compiled at run time; a projected parse through k_str_parse and through H_PARSE.  The group's own contexts are the ones
    its shards run on: the default context's options do not reach them"""
    jit, pk = request.param
    for setter in (ctx.set_option, group.set_option):
        setter("jit", jit); setter("jit_min_rows", 0); setter("parse_kernel", pk)
    yield request.param
    for setter in (ctx.set_option, group.set_option):
        setter("jit", 1); setter("jit_min_rows", 1 << 22); setter("parse_kernel", 1)


def caught(fn):
    try:
        fn()
    except Exception as e:          # noqa: BLE001 — class and text are what is compared
        return type(e).__name__, str(e)
    return None


def healthy(dfdb, gt):
    from dfdb import group as G, ir
    assert G.gnrow(gt.view()[ir.col(1) % 2 == 0, dfdb.ALL]) == (N + 1) // 2


def predicate_calls(dfdb, gt, bad):
    """every entry point that evaluates the view's predicate over the shards"""
    from dfdb import group as G, _native as NAT
    return {"gnrow": lambda: G.gnrow(bad), "gaggregate": lambda: G.gaggregate(bad[dfdb.ALL, ["k"]], NAT.AGG_SUM), "gunique": lambda: G.gunique(bad.s8),
            "ggroupreduce": lambda: G.ggroupreduce(bad, "s8", "k", "sum"), "gindices": lambda: G.gindices(bad)}


# ---------------------------------------------------------------- values
def test_values_over_three_shards(dfdb_mod, ctx, group, tables, mode):
    from dfdb import group as G, _native as NAT, ir
    gt, t1, _ = tables()
    vals, base = tables.vals, tables.base
    k = np.arange(N)
    lo, step, hi = 1000, 3, 8 * BS + 2000                                  # a range stage from shard 0 into shard 2
    in_range = np.zeros(N, bool); in_range[lo - 1:hi:step] = True
    assert shard_of(lo - 1) == 0 and shard_of(hi - 1) == 2
    for name, dtype in (("s", R.I64), ("s8", R.U8), ("sf", R.F64)):
        want = expected(dtype, base[name])
        if dtype == R.F64:
            same_bits(want, np.array([float(x) for x in base[name]], np.float64))
        proj = {"r": (name, lambda s, dtype=dtype: ir.parse(dtype, s))}
        same_bits(G._gq(gt.view()[dfdb_mod.ALL, proj]).materialize()[0], want)
        same_bits(G._gq(gt.view()[ir.col(1) % 10 == 3, dfdb_mod.ALL][dfdb_mod.ALL, proj]).materialize()[0], want[k % 10 == 3])
        same_bits(G._gq(gt.view()[dfdb_mod.jr(lo, step, hi), dfdb_mod.ALL][dfdb_mod.ALL, proj]).materialize()[0], want[in_range])
    c = int(np.median(vals))
    for v, v1, m in ((gt.view()[ir.parse(ir.I64, ir.col(0)) > c, dfdb_mod.ALL], dfdb_mod.DFView(t1)[ir.parse(ir.I64, ir.col(0)) > c, dfdb_mod.ALL], vals > c),
                     (gt.view()[dfdb_mod.jr(lo, step, hi), dfdb_mod.ALL][ir.parse(ir.I64, ir.col(0)) > c, dfdb_mod.ALL],
                      dfdb_mod.DFView(t1)[dfdb_mod.jr(lo, step, hi), dfdb_mod.ALL][ir.parse(ir.I64, ir.col(0)) > c, dfdb_mod.ALL], in_range & (vals > c))):
        assert G.gnrow(v) == int(m.sum())
        assert np.array_equal(G.gindices(v), np.nonzero(m)[0] + 1)
        assert G.gaggregate(v[dfdb_mod.ALL, ["k"]], NAT.AGG_SUM) == int(k[m].sum())
        assert list(G.gunique(v.s)) == list(v1.s.unique()) == list(dict.fromkeys(base["s"][i] for i in np.nonzero(m)[0]))
        w, r = dfdb_mod.groupreduce(v1, "s8", "k", "sum"), G.ggroupreduce(v, "s8", "k", "sum")
        assert list(w["s8"]) == list(r["s8"]) and np.array_equal(w["count"].to_numpy(), r["count"].to_numpy()) and np.array_equal(w["sum"].to_numpy(), r["sum"].to_numpy())
        first = list(dict.fromkeys(base["s8"][i] for i in np.nonzero(m)[0]))
        assert list(r["s8"]) == first and int(r["sum"].sum()) == int(k[m].sum())


# ---------------------------------------------------------------- errors
@pytest.mark.parametrize("shard", range(WORLD))
@pytest.mark.parametrize("kind", KINDS, ids=[KIND_ID[k] for k in KINDS])
def test_each_kind_in_each_shard(dfdb_mod, ctx, group, tables, mode, kind, shard):
    from dfdb import group as G, ir
    row = ROWS[shard]
    assert shard_of(row) == shard and parse_ref(R.I64, SAMPLE[kind])[0] == kind
    gt, t1, _ = tables({row: SAMPLE[kind]})
    pred = ir.parse(ir.I64, ir.col(0)) > 5
    single = caught(lambda: dfdb_mod.DFView(t1)[pred, dfdb_mod.ALL]._query().count())
    assert single is not None and single[0] == EXC[kind].__name__ and re.match("^" + re.escape(PREFIX[kind]) + rf".*\(row {row}\)$", single[1]), single
    bad = gt.view()[pred, dfdb_mod.ALL]
    for name, call in predicate_calls(dfdb_mod, gt, bad).items():
        with raises(kind, row):
            call()
        assert caught(call) == single, name
        healthy(dfdb_mod, gt)
    q = G.GroupQuery(gt, bad)
    try:
        first = caught(q.count_async)                                        # enqueue only: one process owns every shard and may hear of it here already
        assert first in (None, single), first
        with raises(kind, row):
            q.count()
        assert caught(q.count) == single
    finally:
        q.close()
    healthy(dfdb_mod, gt)
    proj = {"r": ("s", lambda s: ir.parse(ir.I64, s))}
    single_m = caught(lambda: dfdb_mod.materialize(dfdb_mod.DFView(t1)[dfdb_mod.ALL, proj]))
    assert single_m == single, (single_m, single)
    for view in (gt.view()[dfdb_mod.ALL, proj], gt.view()[ir.col(1) >= row - 5, dfdb_mod.ALL][dfdb_mod.ALL, proj]):
        with raises(kind, row):
            G._gq(view).materialize()
        assert caught(lambda: G._gq(view).materialize()) == single
        healthy(dfdb_mod, gt)
    # a range stage that ends before the bad row's block: nothing is evaluated there
    if shard == 2:
        end = 8 * BS - 100
        v = gt.view()[dfdb_mod.jr(1, end), dfdb_mod.ALL][ir.parse(ir.I64, ir.col(0)) % 2 == 1, dfdb_mod.ALL]
        m = np.zeros(N, bool); m[:end] = np.fmod(tables.vals[:end], 2) == 1
        assert G.gnrow(v) == int(m.sum()) and np.array_equal(G.gindices(v), np.nonzero(m)[0] + 1)


@pytest.mark.parametrize("first,second", [(OVERFLOW, UNSUPPORTED), (UNSUPPORTED, ARGUMENT), (METHOD, OVERFLOW), (ARGUMENT, METHOD)])
@pytest.mark.parametrize("shards", [(0, 1), (1, 2), (0, 2)])
def test_the_smaller_table_row_decides_between_two_shards(dfdb_mod, ctx, group, tables, mode, first, second, shards):
    from dfdb import group as G, ir
    r1, r2 = ROWS[shards[0]], ROWS[shards[1]]
    gt, t1, _ = tables({r1: SAMPLE[first], r2: SAMPLE[second]})
    pred = ir.parse(ir.I64, ir.col(0)) == 5
    single = caught(lambda: dfdb_mod.DFView(t1)[pred, dfdb_mod.ALL]._query().count())
    bad = gt.view()[pred, dfdb_mod.ALL]
    for name, call in predicate_calls(dfdb_mod, gt, bad).items():
        with raises(first, r1):
            call()
        assert caught(call) == single, name
    with raises(first, r1):
        G._gq(gt.view()[dfdb_mod.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s))}]).materialize()
    healthy(dfdb_mod, gt)


@pytest.mark.parametrize("kind", KINDS, ids=[KIND_ID[k] for k in KINDS])
def test_divide_error_beside_parse_error(dfdb_mod, ctx, group, tables, mode, kind):
    """a zero divisor in an earlier shard wins over a parse error in a later one, and the other way round: as predicates (the fault key: the smaller table
    row) and as two computed columns of a projection (the lowest shard's block comes first)"""
    from dfdb import group as G, ir
    ra, rb = ROWS[1], ROWS[2]
    pred = (ir.parse(ir.I64, ir.col(0)) == 5) & (ir.div(1, ir.col(2)) == 1)
    proj = {"r": ("s", lambda s: ir.parse(ir.I64, s)), "d": (("k", "z"), lambda k, z: ir.div(k, z))}
    for zero_row, bad_row, divide_wins in ((ra, rb, True), (rb, ra, False)):
        gt, t1, _ = tables({bad_row: SAMPLE[kind]}, zeros=(zero_row,))
        single = caught(lambda: dfdb_mod.DFView(t1)[pred, dfdb_mod.ALL]._query().count())
        single_m = caught(lambda: dfdb_mod.materialize(dfdb_mod.DFView(t1)[dfdb_mod.ALL, proj]))
        bad = gt.view()[pred, dfdb_mod.ALL]
        for name, call in predicate_calls(dfdb_mod, gt, bad).items():
            got = caught(call)
            if divide_wins:
                assert got is not None and got[0] == "ZeroDivisionError" and single[0] == "ZeroDivisionError", (name, got, single)
            else:
                with raises(kind, bad_row):
                    call()
                assert got == single, (name, got, single)
            healthy(dfdb_mod, gt)
        got_m = caught(lambda: G._gq(gt.view()[dfdb_mod.ALL, proj]).materialize())
        assert got_m is not None and single_m is not None and got_m[0] == single_m[0], (got_m, single_m)
        if divide_wins:
            assert got_m[0] == "ZeroDivisionError", got_m
        else:
            assert got_m[0] == EXC[kind].__name__ and re.match("^" + re.escape(PREFIX[kind]) + rf".*\(row {bad_row}\)$", got_m[1]) and got_m == single_m, (got_m, single_m)
        healthy(dfdb_mod, gt)


def test_messy_column_row_by_row_over_shards(dfdb_mod, ctx, group, tables, mode):
    """what a real import holds: for a sample of the rows without a value, the selection that starts at that row raises that row's outcome on the group"""
    from dfdb import group as G, ir
    strs = messy_strings(np.random.default_rng(3), N)
    ref = [parse_ref(R.I64, s) for s in strs]
    bad_rows = [i for i, (kd, _) in enumerate(ref) if kd != R.VALUE]
    gt, t1, _ = tables({i: strs[i] for i in range(N)})
    picks = bad_rows[:: max(1, len(bad_rows) // 30)]
    assert {shard_of(r) for r in picks} == {0, 1, 2} and len({ref[r][0] for r in picks}) >= 3
    for row in picks:
        with raises(ref[row][0], row):
            G._gq(gt.view()[ir.col(1) >= row, dfdb_mod.ALL][dfdb_mod.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s))}]).materialize()
    healthy(dfdb_mod, gt)


# ---------------------------------------------------------------- one process per rank: the ranks that do not own the bad row rebuild the error from the fault key
_PARSE_RANK_SCRIPT = r"""
import faulthandler, json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "dataframedbs.jl_amd"))
import numpy as np, torch, torch.distributed as dist
import dfdb
from dfdb import ir, group as G, _native as N
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
g = G.Group.create_rank_torch(0)
assert (g.world, g.nlocal, g.first_rank, g.exchange) == (world, 1, rank, N.EXCHANGE_CALLBACK)
def rec(fn):
    try:
        fn(); return ["none", ""]
    except Exception as e:
        return [type(e).__name__, str(e)]
out = {}
for path in sys.argv[3:]:
    faulthandler.dump_traceback_later(240, exit=True)              # a rank left waiting in an exchange ends itself
    gt = G.GroupTable.open(g, path)
    base = gt.view()
    bad = dfdb.selection(base, ir.parse(ir.I64, ir.col(0)) > 5)
    o = {"rows": gt.shard(0).view()._query().count()}
    o["gnrow"] = rec(lambda: G.gnrow(bad))
    o["gaggregate"] = rec(lambda: G.gaggregate(bad[dfdb.ALL, ["k"]], N.AGG_SUM))
    o["gunique"] = rec(lambda: G.gunique(bad.s8))
    o["ggroupreduce"] = rec(lambda: G.ggroupreduce(bad, "s8", "k", "sum"))
    q = G.GroupQuery(gt, bad)
    o["count_async"] = rec(q.count_async)                          # enqueue only: the failing rank hears of it now ...
    o["count"] = rec(q.count)                                      # ... every rank here
    q.close()
    o["after"] = G.gnrow(dfdb.selection(base, ir.col(1) % 2 == 0)) # the group is fine afterwards
    g.barrier()
    gt.close()
    out[os.path.basename(path)] = o
    faulthandler.cancel_dump_traceback_later()
json.dump(out, open(sys.argv[2] + f".{rank}", "w"))
g.close()
dist.destroy_process_group()
"""


def test_three_processes_agree_on_kind_and_row(oracle, dfdb_mod, ctx, tmp_path):
    """3 ranks on device 0 over gloo; the bad row sits in the LAST rank's block range, so ranks 0 and 1 raise what settle_fault rebuilds from the agreed key:
    the same class, the same text and the same table row as the owning rank, for each of parse's four outcomes"""
    _, base = base_columns()
    row = ROWS[2]
    assert shard_of(row) == WORLD - 1
    paths = []
    for kind in KINDS:
        cols = dict(base)
        cols["s"] = list(base["s"]); cols["s"][row] = SAMPLE[kind]
        assert parse_ref(R.I64, SAMPLE[kind])[0] == kind
        paths.append(str(tmp_path / KIND_ID[kind]))
        write_table(oracle, paths[-1], cols)
    script = tmp_path / "rank_parse.py"
    script.write_text(_PARSE_RANK_SCRIPT)
    port = _free_port()
    procs, logs = [], []
    try:
        for r in range(WORLD):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(WORLD), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            procs.append(subprocess.Popen([sys.executable, str(script), ROOT, str(tmp_path / "out")] + paths, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        logs = [p.communicate(timeout=900)[0].decode(errors="replace") for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill(); p.wait()
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    got = [json.load(open(str(tmp_path / "out") + f".{r}")) for r in range(WORLD)]
    assert [g[KIND_ID[KINDS[0]]]["rows"] for g in got] == [4 * BS, 4 * BS, N - 8 * BS]
    for kind in KINDS:
        per_rank = [g[KIND_ID[kind]] for g in got]
        owner = per_rank[-1]
        pattern = "^" + re.escape(PREFIX[kind]) + rf".*\(row {row}\)$"
        for call in ("gnrow", "gaggregate", "gunique", "ggroupreduce", "count_async", "count"):
            assert owner[call][0] == EXC[kind].__name__ and re.match(pattern, owner[call][1]), (kind, call, owner[call])
        for r, o in enumerate(per_rank[:-1]):                                # the ranks that rebuilt it
            for call in ("gnrow", "gaggregate", "gunique", "ggroupreduce", "count"):
                assert o[call][0] == EXC[kind].__name__ and re.match(pattern, o[call][1]), (kind, r, call, o[call])
                assert o[call] == owner[call], (kind, r, call, o[call], owner[call])
            assert o["count_async"] == ["none", ""], (kind, r, o["count_async"])      # healthy ranks hear of it at their next read
        assert all(o["after"] == (N + 1) // 2 for o in per_rank), kind
