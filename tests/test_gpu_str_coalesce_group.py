"""coalesce over String columns across block-range shards (csrc/group.cpp goes through the per-shard functions): three shards on device 0 with the host
exchange, 10 blocks of 4096 rows with a ragged last one, missing rows in every shard's range.  Materialize and add_column of coalesce(s, "") and
coalesce(s, s2) equal the single-table answer in table order, which equals tests/str_coalesce_cases.py's."""
import numpy as np
import pytest

import str_coalesce_cases as K
from str_coalesce_cases import coalesce_ref, flat
from test_gpu_parse_group import write_table

pytestmark = pytest.mark.gpu
BS, WORLD = 4096, 3
N = 9 * BS + 123                                            # 10 blocks, the last one ragged: shards of 4 / 4 / 2 blocks


def columns():
    k = np.arange(N)
    miss = (k % 7 == 0) | ((k >= 4 * BS - 70) & (k < 4 * BS + 70)) | (k >= 9 * BS + 100)      # every 7th, a run over the shard 0 / 1 boundary, the table's tail
    s = K.with_missing(K.row_strings(N), miss)
    s2 = K.with_missing(K.row_strings(N, salt=5), k % 3 == 0)
    for lo, hi in ((0, 4 * BS), (4 * BS, 8 * BS), (8 * BS, N)):
        assert miss[lo:hi].any() and (miss[lo:hi] & (k[lo:hi] % 3 == 0)).any()                # missing rows, and rows missing on both sides, in every shard
    return {"s": s, "s2": s2, "k": k.astype(np.int64)}


@pytest.fixture(scope="module")
def tables(oracle, dfdb_mod, ctx, tmp_path_factory):
    from dfdb import group as G, _native as NAT
    cols = columns()
    path = str(tmp_path_factory.mktemp("str_coalesce_group") / "t")
    write_table(oracle, path, cols)                           # the String columns are Union{String,Missing}
    g = G.Group.create([0] * WORLD, NAT.EXCHANGE_HOST)
    gt = G.GroupTable.open(g, path)
    t1 = dfdb_mod.open_table(path, ctx=ctx)
    assert gt.nrows == N and [gt.shard(l).view()._query().count() for l in range(WORLD)] == [4 * BS, 4 * BS, N - 8 * BS]
    yield gt, t1, cols
    gt.close(); t1.close(); g.close()


def projections():
    from dfdb import ir
    return {"const": ({"r": ("s", lambda s: ir.coalesce(s, ""))}, lambda c: coalesce_ref(c["s"], b"")),
            "column": ({"r": (("s", "s2"), lambda s, s2: ir.coalesce(s, s2))}, lambda c: coalesce_ref(c["s"], c["s2"]))}


def same(got, want_values):
    ws, wd, wt = flat(want_values)
    assert np.array_equal(got[0], ws) and len(got[1]) == wt and np.array_equal(got[1], wd)


@pytest.mark.parametrize("which", ["const", "column"])
def test_materialize_over_three_shards(dfdb_mod, ctx, tables, which):
    from dfdb import group as G, ir
    gt, t1, cols = tables
    proj, ref = projections()[which]
    want = ref(cols)
    k = cols["k"]
    lo, step, hi = 1000, 3, 8 * BS + 2000                                  # a range stage from shard 0 into shard 2
    in_range = np.zeros(N, bool); in_range[lo - 1:hi:step] = True
    for sel, m in ((None, np.ones(N, bool)), (ir.col(2) % 10 == 3, k % 10 == 3), (dfdb_mod.jr(lo, step, hi), in_range), (ir.col(2) < 0, np.zeros(N, bool))):
        gv, v1 = gt.view(), dfdb_mod.DFView(t1)
        if sel is not None:
            gv, v1 = gv[sel, dfdb_mod.ALL], v1[sel, dfdb_mod.ALL]
        w = [x for x, keep in zip(want, m) if keep]
        single = v1[dfdb_mod.ALL, proj]._query().materialize()[0]
        same(single, w)
        same(G._gq(gv[dfdb_mod.ALL, proj]).materialize()[0], w)


@pytest.mark.parametrize("which", ["const", "column"])
def test_add_column_on_every_shard(dfdb_mod, ctx, tables, which):
    """add_column! of the coalesced column shard by shard (each shard's rows are its block range), then read back through the group in table order"""
    from dfdb import group as G, ir
    gt, t1, cols = tables
    proj, ref = projections()[which]
    want = ref(cols)
    name = "new_" + which
    for l in range(WORLD):
        sh = gt.shard(l)
        sh.add_column_from(name, dfdb_mod.DFView(sh)[dfdb_mod.ALL, proj])
    t1.add_column_from(name, dfdb_mod.DFView(t1)[dfdb_mod.ALL, proj])
    assert gt.shard(0).getmeta(name).type == t1.getmeta(name).type == ("String" if which == "const" else "Missing(String)")
    same(dfdb_mod.DFView(t1)[dfdb_mod.ALL, [name]]._query().materialize()[0], want)
    same(G._gq(gt.view()[dfdb_mod.ALL, [name]]).materialize()[0], want)
    m = cols["k"] % 10 == 3
    same(G._gq(gt.view()[ir.col(2) % 10 == 3, dfdb_mod.ALL][dfdb_mod.ALL, [name]]).materialize()[0], [x for x, keep in zip(want, m) if keep])
    o = gt.shard(0).ordinal(name)
    hit = ir.coalesce(ir.col(o) == "", False)
    assert G.gnrow(gt.view()[hit, dfdb_mod.ALL]) == dfdb_mod.nrow(dfdb_mod.DFView(t1)[hit, dfdb_mod.ALL]) == sum(x == b"" for x in want)
