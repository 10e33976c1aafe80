#!/usr/bin/env python3
"""Legs of dfdb_sort_indices_n (csrc/sort.cpp, k_sort_rekey of csrc/k_sort.hip: the stable sortperm of a selection by several columns), measured on one GPU.

Input: --rows (default 1e9) resident rows at 10 % selectivity (`u100 < 10` on another column), two legs of two keys, the major key first:
  a, r   Int64 below 1e3 (2 of its 8 key bytes vary), Int64 whose every key byte varies (row number x an odd 64-bit constant, wrapping): the
         minor key decides nearly every comparison
  f, z   Float64 (the uniform [0, 2000) generator), a nullable Int32 (one row in 8 missing): the major key has hardly a tie

On an EXECUTED query — the selection bitmap is there, as it is after dfdb_count — every round times, interleaved, whole calls into device memory:

  (m)  dfdb_sort_indices_n by both keys
  (s1) dfdb_sort_indices by the major key alone        (s2) dfdb_sort_indices by the minor key alone

The expectation recorded and judged: (m) costs about (s1) + (s2) — the minor key IS a single-key sort; the major key's sort has the same passes, but its
pairs are built from the row order by k_sort_rekey instead of streamed through the bitmap.  A rekey is one random gather of a value (and, for a nullable
column, of a missing word) per pair: bound by 128-byte lines, not by bytes, so it costs more than the build it replaces.  The line prints (m) / ((s1) + (s2))
and, from one more call with the context's per-launch profiling on, what the rekey launches themselves took.

  (h)  --host-rounds times (default 3: it takes tens of seconds): materialize both columns + np.lexsort on the host — what a caller does without the entry
       point; its row order must equal the device's

(m), (s1), (s2) are timed with HIP events around the whole call, (h) with the host clock.  ROUNDS rounds after a warm-up; the figure is the median, the spread
is max - min.

    python tools/sort_multi_legs.py > profiles/sort_multi.txt
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


def add_nullable_i32(t, name, n):
    """a nullable Int32 column made on the host piece by piece: pseudo-random values, one row in 8 missing (the bytes under the flags stay what they are)"""
    from dfdb import _native as N, ir
    vals, miss = np.empty(n, np.int32), np.empty(n, np.uint8)
    step = 1 << 26
    for lo in range(0, n, step):
        k = np.arange(lo, min(lo + step, n), dtype=np.uint64)
        h = k * np.uint64(0x9E3779B97F4A7C15)
        vals[lo:lo + len(k)] = (h >> np.uint64(32)).astype(np.uint32).view(np.int32)
        miss[lo:lo + len(k)] = ((h >> np.uint64(13)) & np.uint64(7)) == 0
    N.check(N.load().dfdb_table_add_column(t._h, name.encode(), ir.I32 | ir.NULLABLE, n, vals.ctypes.data, None, 0, miss.ctypes.data))


def run_leg(torch, ctx, t, major, minor, host_rounds):
    v = t[("u100", lambda u: u < 10), [major, minor]]
    q = v._query()
    cnt = q.count()                                                    # executes the selection: the bitmap stays
    out = torch.empty(max(cnt, 1), dtype=torch.int64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    info = {}

    def multi():
        info["m"] = q.sort_indices_n([0, 1], None, None, dev_ptr=out.data_ptr(), cap=cnt)[1]

    def single1():
        info["s1"] = q.sort_indices(0, False, None, dev_ptr=out.data_ptr(), cap=cnt)[1]

    def single2():
        info["s2"] = q.sort_indices(1, False, None, dev_ptr=out.data_ptr(), cap=cnt)[1]

    def timed(f):
        ctx.synchronize(); ctx.timer_start(); f(); return ctx.timer_stop()

    for f in (multi, single1, single2):
        f(); f()
    ms = {"m": [], "s1": [], "s2": []}
    for _ in range(ROUNDS):
        ms["s1"].append(timed(single1)); ms["m"].append(timed(multi)); ms["s2"].append(timed(single2))
    m, s1, s2 = med(ms["m"]), med(ms["s1"]), med(ms["s2"])
    ctx.synchronize()
    ctx.profile(True)
    multi()
    ctx.synchronize()
    launches, rekey_ms = ctx.profile_get("sort_rekey")
    ctx.profile(False)
    name = f"{major}, {minor}"
    print(f"{name}  n {cnt:>10d}  (m) both keys {m:8.3f} ms (spread {spread(ms['m']):7.3f}; pairs {info['m'][1]}, passes {info['m'][2]} run {info['m'][3]} skipped)  "
          f"(s1) {major} alone {s1:8.3f} ms (spread {spread(ms['s1']):7.3f}; passes {info['s1'][2]})  (s2) {minor} alone {s2:8.3f} ms (spread {spread(ms['s2']):7.3f}; "
          f"passes {info['s2'][2]})  (m) / ((s1) + (s2)) = {m / (s1 + s2):5.2f}  rekey: {launches} launch(es), {rekey_ms:7.3f} ms in one profiled call "
          f"= {rekey_ms * 1e6 / max(cnt, 1):6.3f} ns per entry", flush=True)
    if not host_rounds:
        return
    multi()
    ctx.synchronize()
    got = out[:cnt].cpu().numpy()
    host = []
    for _ in range(host_rounds):
        t0 = time.perf_counter()
        cols = v._query().materialize()                                # (a query of its own: the scan is part of what the host path costs)
        keys = []
        for a in (cols[1], cols[0]):                                   # (lexsort's LAST key is the major one)
            if np.ma.isMaskedArray(a):
                keys += [a.filled(0), np.ma.getmaskarray(a)]           # missing after the values, like the device
            else:
                keys.append(a)
        order = np.lexsort(tuple(keys))
        host.append((time.perf_counter() - t0) * 1e3)
    rows = q.indices()[order]                                          # (no NaN, no -0.0 in these columns: numpy's order is isless)
    assert np.array_equal(got, rows), (name, got[:8], rows[:8])
    h = med(host)
    verdict = "FASTER by more than the two spreads combined" if h - m > spread(host) + spread(ms["m"]) else "NOT faster by more than the two spreads combined"
    print(f"{name}  n {cnt:>10d}  (h) host materialize + np.lexsort {h:10.1f} ms (spread {spread(host):9.1f}) = {h / m:7.1f} x (m); the two row orders are equal; "
          f"the device is {verdict}", flush=True)


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
    print(f"# {ctx.device_info()['name']}: dfdb_sort_indices_n into device memory, {n} resident rows at 10 % selectivity; whole calls on an executed query, HIP "
          f"events, {ROUNDS} interleaved rounds after a warm-up (median, spread = max - min); every figure measured on this one GPU", flush=True)
    for major, minor in (("a", "r"), ("f", "z")):
        t = dfdb.DFTable.new(block_size=65536, ctx=ctx)                # one pair of key columns at a time beside the selector column
        t.add_generated("u", dfdb.GEN_I64_MOD1M, 13, n)
        t.add_column_from("u100", t[dfdb.ALL, ("u", lambda u: u % 100)])
        if major == "a":
            t.add_generated("i", dfdb.GEN_I64_MOD1M, 11, n)
            t.add_column_from("a", t[dfdb.ALL, ("i", lambda i: i % 1000)])
            t.add_generated("k", dfdb.GEN_I64_IOTA, 0, n)
            t.add_column_from("r", t[dfdb.ALL, ("k", lambda k: k * ODD)])
        else:
            t.add_generated("f", dfdb.GEN_F64_U2000, 12, n)
            add_nullable_i32(t, "z", n)
        run_leg(torch, ctx, t, major, minor, a.host_rounds)
        t.close()


if __name__ == "__main__":
    main()
