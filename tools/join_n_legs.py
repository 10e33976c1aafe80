#!/usr/bin/env python3
"""Legs of dfdb_query_join_n + dfdb_query_join_fetch (csrc/join.cpp, csrc/k_join.hip: the join of two selections on several keys, String keys among them),
measured on one GPU.  Every leg names its yardstick, measured in the same process, interleaved with it.

  (a)  two Int64 keys: a fact table of --rows (default 1e9) rows at 10 % selectivity, keys (a below 1e3, b below 1e3), into their 1e6 unique tuples
         (y1)  dfdb_query_join on ONE precomputed Int64 column a * 1000 + b over the same rows: what a user can do without the entry point
         (y2)  the sort of the right side alone by (a, b) (dfdb_sort_indices_any: dfdb_sort_indices_n's driver)
  (b)  a String key: the brand strings of bench.py's config 4, --rows / 2 rows with a fifth selected, into a ten-row table
         (y1)  dfdb_query_join on an Int64 column of ten values over the same selection (values drawn on their own: as many pairs, not the same pairs)
  (c)  (b) with the String as minor key behind an Int64 key of 1e3 values, into 1e4 tuples
         (y1)  as (b)'s

On EXECUTED queries — both selection bitmaps are there, as they are after dfdb_count — every round times whole calls, join + fetch of both lists into device
memory, with HIP events; ROUNDS interleaved rounds after a warm-up; the figure is the median, the spread is max - min.  One more call with the context's
per-launch profiling on gives the kernels' own times, the refine launch of every stage apart.  --host: materialize of the key columns +
pandas.merge on the host, its pair lists asserted equal to the device's (tens of seconds and tens of GB at full size: run it at a fiftieth).

    python tools/join_n_legs.py > profiles/join_n.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dataframedbs.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ROUNDS = 9
KERNELS = ("join_refine", "join_live", "join_expand", "join_probe", "sort_rows", "sort_rekey", "sort_strkey", "sort_strkey_len", "str_row_offsets", "sort_build", "sort_count",
           "sort_scatter", "sort_order", "scan_counts")
STAGES = tuple(f"join_refine.{k}" for k in range(1, 9)) + ("join_refine.9+",)      # the refine launch of stage 1, 2, .. timed apart (beside the family's sum)


def med(v): return statistics.median(v)
def spread(v): return max(v) - min(v)


def profiled(ctx, call):
    ctx.synchronize()
    ctx.profile(True)
    call()
    ctx.synchronize()
    got = {k: ctx.profile_get(k) for k in KERNELS + STAGES}
    ctx.profile(False)
    return got


def run_leg(torch, dfdb, ctx, name, what, v, w, cols, v1, w1, right_sort, host, same_pairs):
    """v / w: the views of the join on `cols` key columns per side; v1 / w1: the yardstick's views, one Int64 key in projection column 0"""
    ql, qr, q1l, q1r = v._query(), w._query(), v1._query(), w1._query()
    nl, nr = ql.count(), qr.count()                                    # executes the selections: the bitmaps stay
    assert (q1l.count(), q1r.count()) == (nl, nr)
    n, info = ql.join_count_n(qr, cols, cols, dfdb.JOIN_INNER)
    n1, _ = q1l.join_count(q1r, 0, 0, dfdb.JOIN_INNER)
    assert n == n1 or not same_pairs, (name, n, n1)
    dev = torch.device("cuda", 0)
    lt, rt = torch.empty(max(n, 1), dtype=torch.int64, device=dev), torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    l1, r1 = torch.empty(max(n1, 1), dtype=torch.int64, device=dev), torch.empty(max(n1, 1), dtype=torch.int64, device=dev)
    so = torch.empty(max(nr, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def join_n():
        m, _ = ql.join_count_n(qr, cols, cols, dfdb.JOIN_INNER)
        ql.join_fetch(m, (lt.data_ptr(), rt.data_ptr()))

    def join_1():
        m, _ = q1l.join_count(q1r, 0, 0, dfdb.JOIN_INNER)
        q1l.join_fetch(m, (l1.data_ptr(), r1.data_ptr()))

    def sort_right():
        qr.sort_indices_any(cols, None, None, dev_ptr=so.data_ptr(), cap=nr)

    def timed(f):
        ctx.synchronize(); ctx.timer_start(); f(); return ctx.timer_stop()

    fs = {"n": join_n, "1": join_1}
    if right_sort:
        fs["s"] = sort_right
    for f in fs.values():
        f(); f()
    ctx.synchronize()
    if same_pairs:                                                      # the yardstick's key is the tuple packed into one column: the same pair lists
        assert torch.equal(lt[:n], l1[:n]) and torch.equal(rt[:n], r1[:n]), name
    ms = {k: [] for k in fs}
    for _ in range(ROUNDS):
        for k, f in fs.items():
            ms[k].append(timed(f))
    jn, j1 = med(ms["n"]), med(ms["1"])
    line = (f"({name})  {what}: left {nl:>10d}  right {nr:>8d}  pairs {n:>10d} (yardstick {n1})  sub-keys {info[5]}  (n) dfdb_query_join_n + fetch {jn:8.3f} ms (spread {spread(ms['n']):7.3f}; "
            f"right passes {info[4]})  (y1) dfdb_query_join on one Int64 column + fetch {j1:8.3f} ms (spread {spread(ms['1']):7.3f})  (n) / (y1) = {jn / j1:5.2f}")
    if right_sort:
        s = med(ms["s"])
        line += f"  (y2) sort of the right side alone by the same keys {s:8.3f} ms (spread {spread(ms['s']):7.3f})  (n) / (y2) = {jn / s:6.2f}"
    print(line, flush=True)
    pn, p1 = profiled(ctx, join_n), profiled(ctx, join_1)
    print(f"({name})  one profiled call of (n): " + ", ".join(f"{k} {pn[k][0]} x = {pn[k][1]:.3f} ms" for k in KERNELS if pn[k][0]) +
          f";  join_refine per left row and stage {pn['join_refine'][1] * 1e6 / max(nl, 1) / max(pn['join_refine'][0], 1):6.3f} ns", flush=True)
    print(f"({name})  the same call, join_refine by stage (the major sub-key first): " + ", ".join(f"{k.split('.')[1]}: {pn[k][1]:.3f} ms" for k in STAGES if pn[k][0]), flush=True)
    print(f"({name})  one profiled call of (y1): " + ", ".join(f"{k} {p1[k][0]} x = {p1[k][1]:.3f} ms" for k in KERNELS if p1[k][0]) +
          f";  join_probe per left row {p1['join_probe'][1] * 1e6 / max(nl, 1):6.3f} ns", flush=True)
    if not host:
        print(f"({name})  (h) host materialize + pandas.merge: not measured in this run", flush=True)
        return
    import pandas as pd
    gl, gr = lt[:n].cpu().numpy(), rt[:n].cpu().numpy()
    t0 = time.perf_counter()
    sides = [dfdb.materialize(v), dfdb.materialize(w)]                  # (both views project the key columns alone, under the same names)
    on = list(sides[0].columns)
    sides[0]["l"] = np.arange(len(sides[0])); sides[1]["r"] = np.arange(len(sides[1]))
    m = sides[0].merge(sides[1], on=on, how="inner", sort=False)
    h = (time.perf_counter() - t0) * 1e3
    lrows, rrows = ql.indices()[m["l"].to_numpy()], qr.indices()[m["r"].to_numpy()]
    order = np.lexsort((rrows, lrows))                                  # (pandas keeps the left order; within a left row its right order is not promised)
    assert len(lrows) == n and np.array_equal(lrows[order], gl) and np.array_equal(rrows[order], gr), (name, n, len(lrows))
    print(f"({name})  (h) host materialize + pandas.merge {h:10.1f} ms (one run) = {h / jn:7.1f} x (n); the two pair lists are equal", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import dfdb
    ctx = dfdb.default_context(0)
    n = a.rows
    print(f"# {ctx.device_info()['name']}: dfdb_query_join_n + dfdb_query_join_fetch (inner) into device memory against its yardsticks; whole calls on executed "
          f"queries, HIP events, {ROUNDS} interleaved rounds after a warm-up (median, spread = max - min); every figure measured on this one GPU in one process", flush=True)
    ALL = dfdb.ALL
    if "a" in a.legs:
        fact = dfdb.DFTable.new(block_size=65536, ctx=ctx)
        fact.add_generated("u", dfdb.GEN_I64_MOD1M, 13, n)
        fact.add_column_from("u100", fact[ALL, ("u", lambda u: u % 100)])
        fact.add_generated("m", dfdb.GEN_I64_MOD1M, 11, n)
        fact.add_generated("v", dfdb.GEN_I64_MOD1M, 17, n)
        fact.add_column_from("k0", fact[ALL, ("m", lambda m: m % 1000)])
        fact.add_column_from("k1", fact[ALL, ("v", lambda x: x % 1000)])
        fact.add_column_from("ab", fact[ALL, "k0"] * 1000 + fact[ALL, "k1"])
        i = np.arange(1_000_000, dtype=np.int64)
        dim = dfdb.DFTable.from_columns({"k0": i // 1000, "k1": i % 1000, "ab": i}, ctx=ctx)
        sel = ("u100", lambda u: u < 10)
        run_leg(torch, dfdb, ctx, "a", f"two Int64 keys below 1e3, {n} fact rows at 10 %, into their 1e6 unique tuples", fact[sel, ["k0", "k1"]], dim[ALL, ["k0", "k1"]], [0, 1],
                fact[sel, ["ab"]], dim[ALL, ["ab"]], True, a.host, True)
        dim.close()
        fact.close()
    if "b" in a.legs or "c" in a.legs:
        n2 = n // 2
        fact = dfdb.DFTable.new(block_size=65536, ctx=ctx)
        fact.add_generated("u", dfdb.GEN_I64_MOD1M, 13, n2)
        fact.add_column_from("u100", fact[ALL, ("u", lambda u: u % 100)])
        fact.add_generated("s", dfdb.GEN_STR_BRANDS10, 7, n2)
        fact.add_generated("m", dfdb.GEN_I64_MOD1M, 11, n2)
        fact.add_column_from("c", fact[ALL, ("m", lambda m: m % 1000)])
        brands = sorted(set(dfdb.materialize(fact[dfdb.jr(1, 1, 20000), ["s"]])["s"].tolist()))
        assert len(brands) == 10, brands
        # the yardstick's Int64 key: ten values over the same selection (drawn on their own: its pairs are as many, not the same)
        fact.add_generated("w", dfdb.GEN_I64_MOD1M, 19, n2)
        fact.add_column_from("si", fact[ALL, ("w", lambda x: x % 10)])
        sel = ("u100", lambda u: u < 20)
        if "b" in a.legs:
            dim = dfdb.DFTable.from_columns({"s": brands, "si": np.arange(10, dtype=np.int64)}, ctx=ctx)
            run_leg(torch, dfdb, ctx, "b", f"a String key (ten brands), {n2} fact rows with a fifth selected, into a ten-row table", fact[sel, ["s"]], dim[ALL, ["s"]], [0],
                    fact[sel, ["si"]], dim[ALL, ["si"]], False, a.host, False)
            dim.close()
        if "c" in a.legs:
            fact.add_column_from("cs", fact[ALL, "c"] * 10 + fact[ALL, "si"])
            j = np.arange(10_000, dtype=np.int64)
            dim = dfdb.DFTable.from_columns({"c": j // 10, "s": [brands[k] for k in (j % 10).tolist()], "cs": j}, ctx=ctx)
            run_leg(torch, dfdb, ctx, "c", f"(Int64 below 1e3, String brand), {n2} fact rows with a fifth selected, into 1e4 tuples", fact[sel, ["c", "s"]], dim[ALL, ["c", "s"]],
                    [0, 1], fact[sel, ["cs"]], dim[ALL, ["cs"]], False, a.host, False)
            dim.close()
        fact.close()


if __name__ == "__main__":
    main()
