#!/usr/bin/env python3
"""Legs of dfdb_sort_indices (csrc/k_sort.hip: stable radix sortperm over a selection), measured on one GPU.

Input: --rows (default 1e9) resident rows of
  r   Int64, every key byte varies (row number x an odd 64-bit constant, wrapping): 8 digit passes
  i   Int64 below 1e6 (the mod-1e6 generator): 3 passes, 5 skipped
  f   Float64 (the uniform [0, 2000) generator)
  e   an all-equal Int64 column: 0 passes
each at 100 % and at 10 % selectivity (`u100 < 10` on a second column).  On an EXECUTED query — the selection bitmap is there, as it is after dfdb_count —
every round times, interleaved:

  (a) dfdb_sort_indices of every selected row into device memory (no count read back)
  (b) the same with limit = 10 (the top-k cut: a radix select, then a sort of the few candidates)
  (c) a device-to-device copy of 12 bytes per selected row: what ONE pass must at least move — a pass's algorithmic traffic is the pairs read plus the
      pairs written, {8-byte key, 4-byte row} each way.  Printed beside (a): ((a) / passes) / (c)

and at 10 % selectivity (1e8 selected rows of 1e9), --host-rounds times (default 3: it takes seconds):

  (d) materialize + np.argsort(kind="stable") on the host: what a caller does without the entry point; its row order must equal the device's

(a) - (c) are timed with HIP events around the whole call, (d) with the host clock.  ROUNDS rounds after a warm-up; the figure is the median, the spread is
max - min.  The verdict line compares (a) with (d) at 1e8 selected rows: faster means faster by more than the two spreads combined.

    python tools/sort_legs.py > profiles/sort.txt
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
ODD = -7046029254386353131          # 0x9E3779B97F4A7C15 as Int64


def med(v): return statistics.median(v)
def spread(v): return max(v) - min(v)


def run_leg(torch, ctx, col, name, sel, host_rounds, verdicts):
    q = col.view._query()
    cnt = q.count()                                                    # executes the selection: the bitmap stays
    dev = torch.device("cuda", 0)
    out = torch.empty(max(cnt, 1), dtype=torch.int64, device=dev)
    src, dst = torch.empty(max(cnt, 1) * 12, dtype=torch.uint8, device=dev), torch.empty(max(cnt, 1) * 12, dtype=torch.uint8, device=dev)
    src.zero_(); dst.zero_()
    torch.cuda.synchronize()
    info = {}

    def full():
        info["full"] = q.sort_indices(0, False, None, dev_ptr=out.data_ptr(), cap=cnt)[1]

    def top10():
        info["top"] = q.sort_indices(0, False, 10, dev_ptr=out.data_ptr(), cap=cnt)[1]

    def timed(f):
        ctx.synchronize(); ctx.timer_start(); f(); return ctx.timer_stop()

    def copy_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for f in (top10, full, copy_ms):
        f(); f()
    ms_full, ms_top, ms_copy = [], [], []
    for _ in range(ROUNDS):
        ms_top.append(timed(top10)); ms_full.append(timed(full)); ms_copy.append(copy_ms())
    a, b, c = med(ms_full), med(ms_top), med(ms_copy)
    passes = info["full"][2]
    per_pass = f"(a) / passes / (c) = {a / passes / c:5.2f}" if passes else "no pass to compare"
    print(f"{name} {'100 %' if sel is None else f'{sel} %':>6s}  n {cnt:>11d}  (a) sort {a:9.3f} ms (spread {spread(ms_full):8.3f}; pairs {info['full'][1]}, passes {passes} run {info['full'][3]} skipped)  "
          f"(b) limit 10 {b:8.3f} ms (spread {spread(ms_top):7.3f}; pairs {info['top'][1]}, passes {info['top'][2]})  "
          f"(c) copy of 12 B/row {c:8.3f} ms (spread {spread(ms_copy):6.3f}; {cnt * 24 / c / 1e6:7.1f} GB/s read + written)  {per_pass}", flush=True)
    if sel is None or not host_rounds:
        return
    full()
    ctx.synchronize()
    got = out[:cnt].cpu().numpy()
    host = []
    for _ in range(host_rounds):
        t0 = time.perf_counter()
        v = np.asarray(col.materialize())
        order = np.argsort(v, kind="stable")
        host.append((time.perf_counter() - t0) * 1e3)
    rows = q.indices()[order]                                          # (no NaN, no -0.0 in these columns: numpy's order is isless)
    assert np.array_equal(got, rows), (name, sel, got[:8], rows[:8])
    d = med(host)
    faster = d - a > spread(host) + spread(ms_full)
    verdicts.append((name, cnt, a, d, faster))
    print(f"{name} {sel:>4d} %  n {cnt:>11d}  (d) host materialize + np.argsort(stable) {d:10.1f} ms (spread {spread(host):9.1f}) = {d / a:7.1f} x (a); the two row orders are equal", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--host-rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import dfdb
    ctx = dfdb.default_context(0)
    n = a.rows
    print(f"# {ctx.device_info()['name']}: dfdb_sort_indices into device memory, {n} resident rows; whole calls on an executed query, HIP events, {ROUNDS} interleaved "
          f"rounds after a warm-up (median, spread = max - min); every figure measured on this one GPU", flush=True)
    verdicts = []
    for name in ("r", "i", "f", "e"):
        t = dfdb.DFTable.new(block_size=65536, ctx=ctx)                # one value column at a time beside the selector column
        t.add_generated("u", dfdb.GEN_I64_MOD1M, 13, n)
        if name == "r":
            t.add_generated("k", dfdb.GEN_I64_IOTA, 0, n)
            t.add_column_from("r", t[dfdb.ALL, ("k", lambda k: k * ODD)])
        elif name == "i":
            t.add_generated("i", dfdb.GEN_I64_MOD1M, 11, n)
        elif name == "f":
            t.add_generated("f", dfdb.GEN_F64_U2000, 12, n)
        else:
            t.add_column_from("e", t[dfdb.ALL, ("u", lambda u: u * 0 + 7)])      # the all-equal column, made on the device
        t.add_column_from("u100", t[dfdb.ALL, ("u", lambda u: u % 100)])
        run_leg(torch, ctx, t[dfdb.ALL, name], name, None, a.host_rounds, verdicts)
        run_leg(torch, ctx, t[("u100", lambda u: u < 10), name], name, 10, a.host_rounds, verdicts)
        t.close()
    for name, cnt, dev_ms, host_ms, faster in verdicts:
        print(f"# verdict {name}: the full device sort of {cnt} selected rows takes {dev_ms:.3f} ms, the host path {host_ms:.1f} ms: "
              + ("FASTER by more than the two spreads combined" if faster else "NOT faster by more than the two spreads combined"), flush=True)


if __name__ == "__main__":
    main()
