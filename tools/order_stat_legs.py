#!/usr/bin/env python3
"""Legs of dfdb_order_statistics (csrc/k_select.hip: radix select over a selection), measured on one GPU.

Input: --rows (default 1e9) resident rows of an Int64 column (the mod-1e6 generator), a Float64 column (the uniform [0, 2000) generator) and an
all-equal Int64 column (every row a candidate in every pass, every wave's digits uniform), each at 100 % and at 10 % selectivity (`u100 < 10` on a
second column).  On an EXECUTED query — the selection bitmap is there, as it is after dfdb_count — every round times, interleaved:

  (a) dfdb_order_statistics with the two middle ranks (what median asks for): passes x (one stream of the column through the bitmap + one small D2H)
  (b) dfdb_aggregate(SUM) over the same selection: one such stream — the yardstick: a pass reads what SUM reads, so (a) much above passes x (b), beyond
      the two spreads combined, means the histogram is the bound and not HBM
  (c) materialize + np.partition on the host (--host-rounds, default 3: it takes seconds): what a caller does without the entry point

(a) and (b) are timed with HIP events on the engine stream around the whole call, (c) with the host clock.  ROUNDS rounds after a warm-up; the figure is
the median, the spread is min..max.

    python tools/order_stat_legs.py > profiles/order_stat.txt
"""
import argparse
import ctypes as C
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
PEAK_GBPS = 8000.0


def med(v): return statistics.median(v)


def run_column(dfdb, N, ctx, col, name, sel, n, host_rounds):
    """col: the DFColumn under its selection (sel: None = every row, else the percentage selected)"""
    isf = name == "f"
    q = col.view._query()
    cnt = q.count()                                                    # executes the selection: the bitmap stays
    mid = (1 + cnt) // 2
    ranks = np.array([mid, min(mid + 1, cnt)], np.int64)
    oi, of, c3 = np.zeros(2, np.int64), np.zeros(2, np.float64), np.zeros(3, np.int64)
    si, sf = C.c_int64(), C.c_double()
    L = N.load()

    def select():
        N.check(L.dfdb_order_statistics(q._h, 0, ranks.ctypes.data, 2, None if isf else oi.ctypes.data, of.ctypes.data if isf else None, c3.ctypes.data))

    def total():
        N.check(L.dfdb_aggregate(q._h, N.AGG_SUM, 0, C.byref(si), C.byref(sf)))

    def timed(f):
        ctx.synchronize(); ctx.timer_start(); f(); return ctx.timer_stop()

    for f in (select, total):
        f(); f()
    ms_sel, ms_sum = [], []
    for _ in range(ROUNDS):
        ms_sel.append(timed(select)); ms_sum.append(timed(total))
    ctx.profile(True)
    select()
    passes, kernel_ms = ctx.profile_get("select_hist")
    ctx.profile(False)
    host = []
    for _ in range(host_rounds):
        t0 = time.perf_counter()
        v = np.asarray(col.materialize())
        k = sorted({mid - 1, min(mid, cnt - 1)})
        part = np.partition(v, k)
        host.append((time.perf_counter() - t0) * 1e3)
        got = (of if isf else oi)
        assert part[k[0]] == got[0] and part[k[-1]] == got[1], (name, sel, part[k[0]], part[k[-1]], got)      # (no NaN, no -0.0 in these columns: == is exact)
        del v, part
    assert int(c3[0]) == cnt
    a, b = med(ms_sel), med(ms_sum)
    spread = (max(ms_sel) - min(ms_sel)) + passes * (max(ms_sum) - min(ms_sum))
    gb = passes * (cnt * 8 + n / 8) / 1e9
    verdict = "histogram-bound" if a - passes * b > spread and a > 1.25 * passes * b else "within passes x SUM"
    print(f"{name} {'100 %' if sel is None else f'{sel} %':>6s}  n {cnt:>11d}  (a) select {a:8.3f} ms (min {min(ms_sel):8.3f} max {max(ms_sel):8.3f}; {passes} passes, kernels {kernel_ms:8.3f} ms, "
          f"{gb / a * 1e3:7.1f} GB/s = {100 * gb / a * 1e3 / PEAK_GBPS:4.1f} % of peak)  (b) SUM {b:7.3f} ms (min {min(ms_sum):7.3f} max {max(ms_sum):7.3f})  "
          f"(a) / (passes x (b)) = {a / (passes * b):5.2f}  [{verdict}]"
          + (f"  (c) host materialize + np.partition {med(host):10.1f} ms (min {min(host):10.1f} max {max(host):10.1f}) = {med(host) / a:7.1f} x (a)" if host else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--host-rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import dfdb
    from dfdb import _native as N
    ctx = dfdb.default_context(0)
    n = a.rows
    print(f"# {ctx.device_info()['name']}: dfdb_order_statistics, two middle ranks, {n} resident rows; whole calls on an executed query, HIP events, {ROUNDS} interleaved "
          f"rounds after a warm-up; every figure measured on this one GPU")
    for name, make in (("i", lambda t: t.add_generated("i", dfdb.GEN_I64_MOD1M, 11, n)),
                       ("f", lambda t: t.add_generated("f", dfdb.GEN_F64_U2000, 12, n)),
                       ("e", None)):
        t = dfdb.DFTable.new(block_size=65536, ctx=ctx)                # one value column at a time: 8 GB each at 1e9 rows, beside the 8 GB of `u`
        t.add_generated("u", dfdb.GEN_I64_MOD1M, 13, n)
        if make:
            make(t)
        else:
            t.add_column_from("e", t[dfdb.ALL, ("u", lambda u: u * 0 + 7)])      # the all-equal column, made on the device
        t.add_column_from("u100", t[dfdb.ALL, ("u", lambda u: u % 100)])
        run_column(dfdb, N, ctx, t[dfdb.ALL, name], name, None, n, a.host_rounds)
        run_column(dfdb, N, ctx, t[("u100", lambda u: u < 10), name], name, 10, n, a.host_rounds)
        t.close()


if __name__ == "__main__":
    main()
