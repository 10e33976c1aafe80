#!/usr/bin/env python3
"""Legs of the String -> DateTime conversion (the tutorial's `event_time` step: add_column!(t, :time, datetime19.(t.event_time))), measured on one GPU.

Input: --rows (default 1e8) 23-byte strings "yyyy-mm-dd HH:MM:SS UTC", ascending by seconds from 2019-10-01 with about 42 rows per second like the
tutorial's column, built with numpy and handed to dfdb_table_add_column as sizes plus bytes.  The legs run INTERLEAVED, --rounds rounds (default 7) after a
warm-up of each, every call timed with HIP events on the engine stream (dfdb_ctx_timer_*); reported are the median and the spread (max - min) of a leg's
rounds.  The kernels' own times come from the per-launch profile (dfdb_ctx_profile_*) of one more call per leg, outside the rounds.  GB/s counts the
algorithmic bytes per row (4 of size + the string + 8 of result; the scan writes a bit) against the 8 TB/s peak.

  datetime, kernel        add_column of datetime19.(s) into a new resident DateTime column through k_str_convert, datetime conversion (parse_kernel = 1)
  datetime, compiled      the same through the interpreter's H_DATETIME compiled at run time (parse_kernel = 0, jit = 2)
  datetime, interpreted   the same interpreted (parse_kernel = 0, jit = 0)
  parse 19 digits         k_str_convert (parse conversion) over as many 19-digit strings: the README's parse row, in this process
  scan s == const         the String equality count over the timestamp column: the read ceiling for these sizes and bytes

The last line applies the acceptance rule: the kernel stays the default route only if its median is below the compiled interpreter's by more than the two
spreads combined.

    python tools/datetime_legs.py > profiles/datetime.txt
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

LEN, DIGITS = 23, 19
PER_SECOND = 42
PEAK_GBPS = 8000.0


def build_timestamps(n):
    """(sizes, bytes, the first 1000 instants as datetime64[ms]): one formatted row per second, repeated PER_SECOND times"""
    nsec = -(-n // PER_SECOND)
    inst = np.datetime64("2019-10-01T00:00:00", "s") + np.arange(nsec).astype("timedelta64[s]")
    txt = np.datetime_as_string(inst, unit="s").astype("S19").view(np.uint8).reshape(nsec, 19)
    rows = np.empty((nsec, LEN), np.uint8)
    rows[:, :19] = txt
    rows[:, 10] = ord(" ")
    rows[:, 19:] = np.frombuffer(b" UTC", np.uint8)
    data = np.repeat(rows, PER_SECOND, axis=0)[:n].reshape(-1)
    return np.full(n, LEN, np.int32), data, np.repeat(inst[:1000], PER_SECOND)[:1000].astype("datetime64[ms]")


def build_digits(n, rng):
    data = rng.integers(48, 58, (n, DIGITS), dtype=np.uint8)
    data[:, 0] = rng.integers(49, 57, n, dtype=np.uint8)
    return np.full(n, DIGITS, np.int32), data.reshape(-1)


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
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import dfdb
    from dfdb import _native as N
    from dfdb import ir
    n = a.rows
    ctx = dfdb.default_context(0)
    ctx.set_option("jit_min_rows", 0)
    L = N.load()
    sizes, data, head = build_timestamps(n)
    t = dfdb.DFTable.new(block_size=65536)
    N.check(L.dfdb_table_add_column(t._h, b"s", ir.STRING, n, sizes.ctypes.data, data.ctypes.data, len(data), None))
    probe = bytes(data[:LEN]).decode()
    sizes, data = build_digits(n, np.random.default_rng(1))
    td = dfdb.DFTable.new(block_size=65536)
    N.check(L.dfdb_table_add_column(td._h, b"s", ir.STRING, n, sizes.ctypes.data, data.ctypes.data, len(data), None))
    del sizes, data
    print(f"# {ctx.device_info()['name']}: {n} rows; {LEN}-byte timestamps ascending by seconds ({PER_SECOND} rows per second), {DIGITS}-digit strings for the parse leg;")
    print(f"# block size 65536; {a.rounds} interleaved rounds after a warm-up of each leg, HIP events; median, +- spread (max - min)")
    added = [0]

    def add_dt():
        added[0] += 1
        t.add_column(f"dt{added[0]}", dfdb.datetime19(dfdb.DFView(t).s))

    def add_parse():
        added[0] += 1
        td.add_column_from(f"id{added[0]}", dfdb.DFView(td)[dfdb.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s))}])

    def scan():
        return dfdb.DFView(t)[ir.col(0) == probe, dfdb.ALL]._query().count()

    #        name                                   options (parse_kernel, jit)  call       bytes per row
    legs = [("datetime19 add_column, kernel", (1, 2), add_dt, 4 + LEN + 8),
            ("datetime19 add_column, interpreter compiled", (0, 2), add_dt, 4 + LEN + 8),
            ("datetime19 add_column, interpreter interpreted", (0, 0), add_dt, 4 + LEN + 8),
            (f"parse(Int64, s) add_column, {DIGITS} digits, kernel", (1, 2), add_parse, 4 + DIGITS + 8),
            (f"scan: count(s == \"{probe}\")", (1, 2), scan, 4 + LEN)]

    def run(leg, timed=True):
        _, (pk, jit), fn, _ = leg
        ctx.set_option("parse_kernel", pk)
        ctx.set_option("jit", jit)
        if not timed:
            return fn()
        ctx.synchronize()
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    for leg in legs:
        run(leg, timed=False)                                   # warm-up: compiles, allocates
    times = [[] for _ in legs]
    for _ in range(a.rounds):
        for i, leg in enumerate(legs):
            times[i].append(run(leg))
    got = dfdb.materialize(dfdb.DFView(t)[dfdb.jr(1, 1000), dfdb.ALL][dfdb.ALL, ["dt1"]])["dt1"].to_numpy().astype("datetime64[ms]")
    assert np.array_equal(got, head), "the converted column differs from numpy's reading of the same strings"
    assert t.getmeta("dt1").type == "DateTime"
    names = ["str_datetime", "str_parse", "jit_project", "interp_project", "str_match"]
    med, spread = [], []
    for i, leg in enumerate(legs):
        med.append(statistics.median(times[i])); spread.append(max(times[i]) - min(times[i]))
        line(leg[0], med[i], spread[i], n, leg[3])
        print("    rounds: " + " ".join(f"{x:.3f}" for x in times[i]))
        for k, (cnt, kms) in kernel_ms(ctx, lambda: run(leg, timed=False), names).items():
            line(f"    kernel {k} x{cnt} (one more call)", kms, None, n, leg[3])
    ctx.set_option("parse_kernel", 1)
    print("# the tutorial's figure for the same conversion: 2.54 MRows/s (43 s for 1.1e8 rows), which includes a disk write on one CPU core: context only")
    margin = spread[0] + spread[1]
    verdict = "kernel stays the default route" if med[0] < med[1] - margin else "kernel does NOT clear the rule: the interpreter should be the default route"
    print(f"# acceptance: kernel median {med[0]:.3f} ms vs compiled interpreter {med[1]:.3f} ms, combined spread {margin:.3f} ms -> {verdict}")


if __name__ == "__main__":
    main()
