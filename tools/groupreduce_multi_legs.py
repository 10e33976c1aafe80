#!/usr/bin/env python3
"""groupreduce by a tuple of keys with several reducers (dfdb_query_groupreduce_n) at 1e9 resident rows: one JSON line per leg and repetition with the
wall ms, the groups, the per-pass device ms of the profile and a bytes-moved estimate against 8 TB/s.
  (a) Int64 key, 5000 groups, 3 reducers (sum Float64, max Int64, count): one _n call, and the three single calls it replaces, in the same process
  (b) keys (Int64, 1000 values) x (String with a dictionary, 10 values), 2 reducers
  (c) two Int64 keys, 1e6 composite groups, 2 reducers
  (d) (c) with one tuple holding 30 % of the rows (the global form's hot slots)
--streamed runs one other leg instead, where the host's by-key merge of the chunks lives (csrc/ooc.cpp GroupMerger): an Int64 key with 1e6 distinct values over a
table saved to files and opened without loading it (DFDB_LEGS_STREAM_ROWS rows, 1e8 by default: every chunk of 512 blocks brings ~1e6 groups to the merge), once
through groupreduce(v, "k", "f", "sum") and once through groupreduce(v, ("k",), s=("f", "sum"), m=("x", "max")).
DFDB_LEGS_REPS repetitions per leg (3 by default; the first one warms up)."""
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dataframedbs.jl_amd")]
import torch  # noqa: E402  (torch's HIP runtime first: see tests/conftest.py)
torch.cuda.init()
import dfdb  # noqa: E402
from dfdb import ir  # noqa: E402

N = int(os.environ.get("DFDB_LEGS_ROWS", 1_000_000_000))
REPS = int(os.environ.get("DFDB_LEGS_REPS", 3))
N_STREAM = int(os.environ.get("DFDB_LEGS_STREAM_ROWS", 100_000_000))
PASSES = ("unique", "unique_insert", "unique_mark", "unique_presence", "unique_first", "unique_minmax", "group_rank", "group_accumulate", "group_accumulate_multi",
          "dict_scan")
ctx = dfdb.default_context(0)


def est_bytes(nkeys, key_widths, val_widths):
    """per row: every key read once by unique and once by the rank pass, G written (4) per key, image written and read back twice per later key (8 x 3),
    then the accumulate pass: G (4) + the value columns + the selection bits"""
    per_row = sum(2 * w for w in key_widths) + 4 * nkeys + 24 * (nkeys - 1) + 4 + sum(val_widths) + 0.125
    return per_row * N


def leg(label, fn, nbytes, rows=N):
    for rep in range(REPS):
        ctx.profile(True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        g = fn()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        prof = {k: round(v[1], 3) for k in PASSES for v in [ctx.profile_get(k)] if v[0]}
        ctx.profile(False)
        print(json.dumps({"leg": label, "rep": rep, "rows": rows, "ms": round(dt * 1e3, 3), "groups": len(g), "bytes_est": int(nbytes),
                          "ms_at_8TBps": round(nbytes / 8e12 * 1e3, 3), "passes_ms": prof}), flush=True)


def streamed():
    t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    t.add_generated("k", dfdb.GEN_I64_MOD1M, 0x9E3779B97F4A7C15, N_STREAM)
    t.add_generated("x", dfdb.GEN_I64_MOD1M, 0x9E3779B97F4A7C15 * 5, N_STREAM)
    t.add_column_from("f", t.k * 0.5)
    d = tempfile.mkdtemp(prefix="dfdb_legs_")
    try:
        t.save(os.path.join(d, "tb"))
        t.close()
        lazy = dfdb.open_table(os.path.join(d, "tb"), load=False, ctx=ctx)
        leg("s: streamed, Int64 key of 1e6 values, single-key call", lambda: dfdb.groupreduce(lazy, "k", "f", "sum"), 16 * N_STREAM, N_STREAM)
        leg("s: streamed, the same key, one _n call with 2 reducers", lambda: dfdb.groupreduce(lazy, ("k",), s=("f", "sum"), m=("x", "max")), 24 * N_STREAM, N_STREAM)
        assert not lazy.resident(0)
        lazy.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


if "--streamed" in sys.argv[1:]:
    streamed()
    sys.exit(0)

t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
t.add_generated("x", dfdb.GEN_I64_MOD1M, 0x9E3779B97F4A7C15, N)
t.add_column_from("k", t.x % 5000)
t.add_column_from("f", t.x * 0.5)
leg("a: 1 key x 3 reducers, one _n call", lambda: dfdb.groupreduce(t, ("k",), s=("f", "sum"), m=("x", "max"), n=("x", "count")), est_bytes(1, [8], [8, 8]))
leg("a: the 3 single calls it replaces", lambda: [dfdb.groupreduce(t, "k", "f", "sum"), dfdb.groupreduce(t, "k", "x", "max"), dfdb.groupreduce(t, "k")][0],
    3 * est_bytes(1, [8], [8]))
t.close()

t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
t.add_generated("x", dfdb.GEN_I64_MOD1M, 0x9E3779B97F4A7C15, N)
t.add_generated("s", dfdb.GEN_STR_BRANDS10, 0x9E3779B97F4A7C15 * 3, N)
t.build_dictionary("s")
t.add_column_from("k", t.x % 1000)
t.add_column_from("f", t.x * 0.5)
leg("b: (Int64 1000) x (dictionary String 10), 2 reducers", lambda: dfdb.groupreduce(t, ("k", "s"), fs=("f", "sum"), xm=("x", "min")), est_bytes(2, [8, 2], [8, 8]))
t.close()

t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
t.add_generated("x", dfdb.GEN_I64_MOD1M, 0x9E3779B97F4A7C15, N)
t.add_generated("h", dfdb.GEN_I64_MOD1M, 0x9E3779B97F4A7C15 * 5, N)
t.add_column_from("k1", t.x % 1000)
t.add_column_from("k2", t.x._bc(ir.IDIV, 1000))                    # x ÷ 1000
t.add_column_from("f", t.x * 0.5)
leg("c: two Int64 keys, 1e6 composite groups, 2 reducers", lambda: dfdb.groupreduce(t, ("k1", "k2"), s=("f", "sum"), m=("x", "max")), est_bytes(2, [8, 8], [8, 8]))
t.add_column_from("g", (t.h + 700_000)._bc(ir.IDIV, 1_000_000))        # 0 for the 30 % of rows with h < 300 000, else 1
t.add_column_from("h1", t.k1 * t.g)
t.add_column_from("h2", t.k2 * t.g)
leg("d: (c) with the tuple (0, 0) in 30 % of the rows", lambda: dfdb.groupreduce(t, ("h1", "h2"), s=("f", "sum"), m=("x", "max")), est_bytes(2, [8, 8], [8, 8]))
t.close()
