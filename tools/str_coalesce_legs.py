#!/usr/bin/env python3
"""Legs of the String -> String conversion (the tutorial's string_convert step: add_column!(t, :s2, coalesce.(t.s, ""))), measured on one GPU.

Input: --rows (default 1e8) of config 4's strings (the ten brands of csrc/k_gen.hip, drawn uniformly), every 7th row missing, in a Union{String,Missing}
column.  The column is built with numpy as one period of 700 000 rows repeated (the draw is uniform, so the repetition changes no length statistic) and
handed to dfdb_table_add_column as sizes plus bytes.  The legs run INTERLEAVED, --rounds rounds (default 9) after a warm-up of each, every call timed with
HIP events on the engine stream (dfdb_ctx_timer_*); reported are the median and the spread (max - min) of a leg's rounds.  The kernels' own times come
from the per-launch profile (dfdb_ctx_profile_*) of one more call per leg, outside the rounds.  GB/s counts the algorithmic bytes per row (4 of size in, the
bytes in, 4 of size out, the bytes out) against the 8 TB/s peak.

  plain copy              add_column of the column s itself into a new resident column (K6: k_str_gather_sizes / _bytes in the plain form): the baseline; it
                          moves the same sizes and the same bytes
  coalesce(s, "")         add_column of coalesce.(s, "") (the same kernel pair in the constant form; profile names str_coalesce_sizes / _bytes)
  coalesce(s, s2)         add_column of coalesce.(s, s2), s2 a second column of the same strings shifted by one row (the two-column form: 4 KB more LDS per wave)

The last line applies the expectation: the coalesce leg's median lies within the two spreads combined of the plain copy's; a larger gap means the per-row
source select costs something.

    python tools/str_coalesce_legs.py > profiles/str_coalesce.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dataframedbs.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BRANDS = [b"apple", b"samsung", b"huawei", b"microsoft", b"dell", b"xbox", b"sony", b"intel", b"lenovo", b"asus"]
PERIOD = 700_000
PEAK_GBPS = 8000.0


def build_column(n, seed, missing_every=7):
    """(sizes with -1 on every 7th row, bytes): one period of PERIOD rows, repeated"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(BRANDS), PERIOD)
    vals = [None if missing_every and i % missing_every == 0 else BRANDS[k] for i, k in enumerate(pick.tolist())]
    psz = np.array([-1 if v is None else len(v) for v in vals], np.int32)
    pby = np.frombuffer(b"".join(v for v in vals if v is not None), np.uint8)
    reps, rest = divmod(n, PERIOD)
    sizes = np.concatenate([np.tile(psz, reps), psz[:rest]])
    tail = int(np.where(psz[:rest] > 0, psz[:rest], 0).sum())
    data = np.concatenate([np.tile(pby, reps), pby[:tail]])
    return sizes, data, vals


def kernel_ms(ctx, fn, names):
    ctx.profile(True)
    before = {k: ctx.profile_get(k) for k in names}
    fn()
    got = {k: ctx.profile_get(k) for k in names}
    ctx.profile(False)
    return {k: (v[0] - before[k][0], v[1] - before[k][1]) for k, v in got.items() if v[0] > before[k][0]}


def line(name, ms, spread, rows, bytes_per_row):
    gbps = rows * bytes_per_row / ms / 1e6
    sp = f"+-{spread:7.3f}" if spread is not None else " " * 9
    print(f"{name:<52s} {ms:9.3f} ms {sp}  {rows / ms / 1e3:10.1f} MRows/s  {gbps:8.1f} GB/s  {100 * gbps / PEAK_GBPS:5.1f} % of peak")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import dfdb
    from dfdb import _native as N
    from dfdb import ir
    n = a.rows
    ctx = dfdb.default_context(0)
    L = N.load()
    t = dfdb.DFTable.new(block_size=65536)
    sizes, data, vals = build_column(n, 1)
    N.check(L.dfdb_table_add_column(t._h, b"s", ir.STRING | ir.NULLABLE, n, sizes.ctypes.data, data.ctypes.data, len(data), None))
    in_bytes = len(data) / n
    sizes2, data2, vals2 = build_column(n, 2, missing_every=0)
    N.check(L.dfdb_table_add_column(t._h, b"s2", ir.STRING, n, sizes2.ctypes.data, data2.ctypes.data, len(data2), None))
    in2_bytes = len(data2) / n
    del sizes, data, sizes2, data2
    print(f"# {ctx.device_info()['name']}: {n} rows of the ten brands, every 7th row of s missing ({in_bytes:.2f} bytes per row), s2 without missing rows ({in2_bytes:.2f});")
    print(f"# block size 65536; {a.rounds} interleaved rounds after a warm-up of each leg, HIP events; median, +- spread (max - min)")
    added = [0]

    def add(col):
        def f():
            added[0] += 1
            t.add_column_from(f"c{added[0]}", col())
            return f"c{added[0]}"
        return f

    v = lambda: dfdb.DFView(t)                                   # noqa: E731
    # the bytes a leg moves per row: size in, bytes in, size out, bytes out (a filled row brings none for "", b's bytes for s2)
    out_const = in_bytes
    out_two = in_bytes + in2_bytes / 7
    legs = [("plain copy: add_column of s", add(lambda: v().s), 8 + 2 * in_bytes),
            ('coalesce(s, ""): add_column', add(lambda: dfdb.coalesce(v().s, "")), 8 + in_bytes + out_const),
            ("coalesce(s, s2): add_column", add(lambda: dfdb.coalesce(v().s, v().s2)), 12 + in_bytes + in2_bytes / 7 + out_two)]

    def run(leg, timed=True):
        if not timed:
            return leg[1]()
        ctx.synchronize()
        ctx.timer_start()
        leg[1]()
        return ctx.timer_stop()

    firsts = [run(leg, timed=False) for leg in legs]             # warm-up: allocates; its columns are checked below
    times = [[] for _ in legs]
    for _ in range(a.rounds):
        for i, leg in enumerate(legs):
            times[i].append(run(leg))
            # every call adds a resident column: drop nothing, the table holds rounds x legs of them (1e8 rows: ~1 GB each)
    head = dfdb.DFView(t)[dfdb.jr(1, 2000), dfdb.ALL][dfdb.ALL, firsts]._query().materialize()
    want = [vals[:2000], [b"" if x is None else x for x in vals[:2000]], [y if x is None else x for x, y in zip(vals[:2000], vals2[:2000])]]
    for (gs, gb), w in zip(head, want):
        assert gs.tolist() == [-1 if x is None else len(x) for x in w] and gb.tobytes() == b"".join(x for x in w if x is not None), "the new column differs from the input lists"
    names = ["str_gather_sizes", "str_gather_bytes", "str_coalesce_sizes", "str_coalesce_bytes", "scan_counts", "str_tile_bytes"]
    med, spread = [], []
    for i, leg in enumerate(legs):
        med.append(statistics.median(times[i])); spread.append(max(times[i]) - min(times[i]))
        line(leg[0], med[i], spread[i], n, leg[2])
        print("    rounds: " + " ".join(f"{x:.3f}" for x in times[i]))
        for k, (cnt, kms) in kernel_ms(ctx, lambda: run(leg, timed=False), names).items():
            line(f"    kernel {k} x{cnt} (one more call)", kms, None, n, leg[2])
    print("# the tutorial's figure for the same conversion: 17.9 MRows/s on one CPU core: context only")
    for i in (1, 2):
        margin = spread[0] + spread[i]
        gap = med[i] - med[0]
        verdict = "within the two spreads combined" if abs(gap) <= margin else "OUTSIDE the two spreads combined: the per-row source select costs (or saves) something, see the kernel lines"
        print(f"# expectation: {legs[i][0]} median {med[i]:.3f} ms vs plain copy {med[0]:.3f} ms, gap {gap:+.3f} ms, combined spread {margin:.3f} ms -> {verdict}")


if __name__ == "__main__":
    main()
