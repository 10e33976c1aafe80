#!/usr/bin/env python3
"""Legs of dfdb_query_join + dfdb_query_join_fetch (csrc/join.cpp, csrc/k_join.hip: the row lists of a join of two selections on one key), measured on one GPU.

Input: a fact table of --rows (default 1e9) resident rows at 10 % selectivity (`u100 < 10` on another column), joined INNER into a dimension table:
  (a)  fact key Int64 below 1e6 (the MOD1M generator)            into 1e6 rows of unique keys 1 .. 1e6          (about one pair per probe)
  (b)  fact key Int64 = the row number 1 .. rows                  into rows / 10 rows of unique keys 10, 20, ..  (one probe in ten has a pair; both sides 1e8)
  (c)  (a)'s fact key                                             into 4e6 rows, every key 0 .. 1e6 - 1 four times (four pairs per probe)

On EXECUTED queries — both selection bitmaps are there, as they are after dfdb_count — every round times, interleaved, whole calls into device memory:

  (j)  dfdb_query_join + dfdb_query_join_fetch of both lists
  (s)  dfdb_sort_indices of the right selection by its key alone: the part of (j) that is existing code
  (r)  dfdb_sort_indices_n over the LEFT selection by (u100, key): its k_sort_rekey makes ONE random gather per entry, where the probe makes up to
       2 x bitlength(right rows) dependent gathers per entry.  From one more call of each with the context's per-launch profiling on the line prints what the
       probe and the rekey launches themselves took per entry and their ratio — the number that decides whether a hash or fence-array probe is worth building
       

  (h)  --host-legs (default "a"; it takes tens of seconds and tens of GB): materialize both key columns + pandas.merge(how="inner") on the host — what a caller
       does without the entry point; its pairs must equal the device's

(j), (s), (r) are timed with HIP events around the whole call, (h) with the host clock.  ROUNDS rounds after a warm-up; the figure is the median, the spread
is max - min.

    python tools/join_legs.py > profiles/join.txt
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


def med(v): return statistics.median(v)
def spread(v): return max(v) - min(v)


def profiled(ctx, names, call):
    ctx.synchronize()
    ctx.profile(True)
    call()
    ctx.synchronize()
    got = {k: ctx.profile_get(k) for k in names}
    ctx.profile(False)
    return got


def run_leg(torch, dfdb, ctx, name, fact, key, dim, host):
    v = fact[("u100", lambda u: u < 10), [key, "u100"]]
    w = dim[dfdb.ALL, "k"].view
    ql, qr = v._query(), w._query()
    nl, nr = ql.count(), qr.count()                                    # executes both selections: the bitmaps stay
    n, info = ql.join_count(qr, 0, 0, dfdb.JOIN_INNER)
    dev = torch.device("cuda", 0)
    lt, rt = torch.empty(max(n, 1), dtype=torch.int64, device=dev), torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    so = torch.empty(max(nl, nr, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    inf = {}

    def join():
        m, inf["j"] = ql.join_count(qr, 0, 0, dfdb.JOIN_INNER)
        ql.join_fetch(m, (lt.data_ptr(), rt.data_ptr()))

    def right_sort():
        inf["s"] = qr.sort_indices(0, False, None, dev_ptr=so.data_ptr(), cap=nr)[1]

    def left_two_keys():
        inf["r"] = ql.sort_indices_n([1, 0], None, None, dev_ptr=so.data_ptr(), cap=nl)[1]      # (key the minor one: u100 is rekeyed from an order the key's sort left)

    def timed(f):
        ctx.synchronize(); ctx.timer_start(); f(); return ctx.timer_stop()

    for f in (join, right_sort, left_two_keys):
        f(); f()
    ms = {"j": [], "s": [], "r": []}
    for _ in range(ROUNDS):
        ms["s"].append(timed(right_sort)); ms["j"].append(timed(join)); ms["r"].append(timed(left_two_keys))
    j, s, r = med(ms["j"]), med(ms["s"]), med(ms["r"])
    pj = profiled(ctx, ("join_probe", "join_expand", "sort_rows", "sort_build", "sort_count", "sort_scatter", "scan_counts"), join)
    pr = profiled(ctx, ("sort_rekey",), left_two_keys)
    probe_ns, rekey_ns = pj["join_probe"][1] * 1e6 / max(nl, 1), pr["sort_rekey"][1] * 1e6 / max(nl, 1)
    steps = int(nr).bit_length()
    print(f"({name})  left {nl:>10d} of {fact_rows(fact):>10d}  right {nr:>9d}  pairs {n:>10d}  (j) join + fetch {j:8.3f} ms (spread {spread(ms['j']):7.3f}; right passes "
          f"{inf['j'][4]})  (s) right sort alone {s:8.3f} ms (spread {spread(ms['s']):7.3f})  (r) left sort by two keys {r:8.3f} ms (spread {spread(ms['r']):7.3f})", flush=True)
    print(f"({name})  one profiled call: join_probe {pj['join_probe'][1]:8.3f} ms = {probe_ns:6.3f} ns per left row ({steps} search steps, 2 searches), join_expand "
          f"{pj['join_expand'][1]:8.3f} ms = {pj['join_expand'][1] * 1e6 / max(n, 1):6.3f} ns per pair, sort_rows {pj['sort_rows'][1]:7.3f}, right side: sort_build "
          f"{pj['sort_build'][1]:7.3f} + {pj['sort_count'][0]} passes {pj['sort_count'][1] + pj['sort_scatter'][1]:7.3f}, scans {pj['scan_counts'][1]:6.3f};  "
          f"sort_rekey {pr['sort_rekey'][1]:8.3f} ms = {rekey_ns:6.3f} ns per entry;  probe / rekey per entry = {probe_ns / max(rekey_ns, 1e-9):5.2f}", flush=True)
    if not host:
        print(f"({name})  (h) host materialize + pandas.merge: not measured in this run", flush=True)
        return
    import pandas as pd
    join()
    ctx.synchronize()
    gl, gr = lt[:n].cpu().numpy(), rt[:n].cpu().numpy()
    t0 = time.perf_counter()
    lk = fact[("u100", lambda u: u < 10), [key]]._query().materialize()[0]      # (queries of their own: the scans are part of what the host path costs)
    rk = dim[dfdb.ALL, "k"].view._query().materialize()[0]
    m = pd.DataFrame({"k": lk, "l": np.arange(len(lk))}).merge(pd.DataFrame({"k": rk, "r": np.arange(len(rk))}), on="k", how="inner", sort=False)
    h = (time.perf_counter() - t0) * 1e3
    lrows, rrows = ql.indices()[m["l"].to_numpy()], qr.indices()[m["r"].to_numpy()]
    order = np.lexsort((rrows, lrows))                                  # (pandas keeps the left order; within a left row its right order is not promised)
    same = len(lrows) == n and np.array_equal(lrows[order], gl) and np.array_equal(rrows[order], gr)
    assert same, (name, n, len(lrows))
    print(f"({name})  (h) host materialize + pandas.merge {h:10.1f} ms (one run) = {h / j:7.1f} x (j); the two pair lists are equal", flush=True)


def fact_rows(t):
    import ctypes as C
    from dfdb import _native as N
    n = C.c_int64()
    N.check(N.load().dfdb_table_nrows(t._h, C.byref(n)))
    return n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--host-legs", default="a")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import dfdb
    ctx = dfdb.default_context(0)
    n = a.rows
    print(f"# {ctx.device_info()['name']}: dfdb_query_join + dfdb_query_join_fetch (inner) into device memory, a fact table of {n} resident rows at 10 % selectivity; whole "
          f"calls on executed queries, HIP events, {ROUNDS} interleaved rounds after a warm-up (median, spread = max - min); every figure measured on this one GPU", flush=True)
    fact = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    fact.add_generated("u", dfdb.GEN_I64_MOD1M, 13, n)
    fact.add_column_from("u100", fact[dfdb.ALL, ("u", lambda u: u % 100)])
    fact.add_generated("m", dfdb.GEN_I64_MOD1M, 11, n)
    fact.add_generated("i", dfdb.GEN_I64_IOTA, 0, n)
    dims = {"a": (1_000_000, lambda k: k * 1, "m"), "b": (max(n // 10, 1), lambda k: k * 10, "i"), "c": (4_000_000, lambda k: k % 1_000_000, "m")}
    for leg in a.legs:
        rows, f, key = dims[leg]
        dim = dfdb.DFTable.new(block_size=65536, ctx=ctx)
        dim.add_generated("i", dfdb.GEN_I64_IOTA, 0, rows)
        dim.add_column_from("k", dim[dfdb.ALL, ("i", f)])
        run_leg(torch, dfdb, ctx, leg, fact, key, dim, leg in a.host_legs)
        dim.close()
    fact.close()


if __name__ == "__main__":
    main()
