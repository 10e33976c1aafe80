#!/usr/bin/env python3
"""dfdb_sort_indices of 1e9 rows called back to back in a process that does nothing else: the per-call times (HIP events and the host clock around the whole
call) of six calls after a warm-up, then one call with per-launch profiling on (launches, summed ms per kernel family).  For a Float64 column (uniform
[0, 2000)) and an Int64 column whose every key byte varies (row number x an odd 64-bit constant, wrapping), 8 digit passes each.  The companion of
tools/sort_legs.py, whose interleaved legs show calls of seconds at this size that this tool does not.

    python tools/sort_back_to_back.py > profiles/sort_back_to_back.txt
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dataframedbs.jl_amd")):
    sys.path.insert(0, p)
import torch
torch.cuda.init()
import dfdb
ctx = dfdb.default_context(0)
n = 1_000_000_000
ODD = -7046029254386353131
for name in ("f", "r"):
    t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    if name == "r":
        t.add_generated("k", dfdb.GEN_I64_IOTA, 0, n)
        t.add_column_from("r", t[dfdb.ALL, ("k", lambda k: k * ODD)])
    else:
        t.add_generated("f", dfdb.GEN_F64_U2000, 12, n)
    q = t[dfdb.ALL, name].view._query()
    cnt = q.count()
    out = torch.empty(cnt, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    def full():
        return q.sort_indices(0, False, None, dev_ptr=out.data_ptr(), cap=cnt)[1]
    full()
    rounds = []
    for _ in range(6):
        ctx.synchronize(); ctx.timer_start(); t0 = time.perf_counter(); full(); ms = ctx.timer_stop(); rounds.append((round(ms, 1), round((time.perf_counter() - t0) * 1e3, 1)))
    print(name, "rounds (event ms, host ms):", rounds, flush=True)
    ctx.profile(True)
    full()
    print(name, "kernels:", {k: ctx.profile_get(k) for k in ("sort_build", "sort_count", "scan_counts", "sort_scatter", "sort_emit")}, flush=True)
    ctx.profile(False)
    del out
    t.close()
