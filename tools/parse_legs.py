#!/usr/bin/env python3
"""Legs of the String -> Int64 conversion (the tutorial's `add_column!(t, :category_id, parse.(Int64, t.category_id_raw))`), measured on one GPU.

Input: --rows (default 1e8) 19-digit decimal strings built with numpy and handed to dfdb_table_add_column as sizes plus bytes, and an Int64 row number
beside them for the 10 % selection.  Every leg is timed with HIP events on the engine stream (dfdb_ctx_timer_*), best of five after a warm-up; the
kernel's own time comes from the per-launch profile (dfdb_ctx_profile_*) of one more run.  GB/s counts (4 + len + 8) bytes per row against the 8 TB/s peak.

  add_column_from   parse(Int64, s) of every row into a new resident column: the conversion kernel k_str_convert (parse conversion), and the interpreter form of the same
                    expression (ctx option parse_kernel = 0) as its run-time compiled kernel (jit = 2) and interpreted (jit = 0)
  materialize 10 %  the selection `k % 10 == 3` executed beforehand, then the parsed column of the selected rows delivered to the host
  yardstick         the String equality scan `s == "<a value>"` over the same column: reads the same sizes and bytes, writes a bitmap

    python tools/parse_legs.py > profiles/parse.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dataframedbs.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LEN = 19
PEAK_GBPS = 8000.0


def build_column(n, rng):
    """n 19-digit strings below 2^63: first digit 1-8, the rest 0-9; returns (sizes, bytes, the values of the first 1000 rows)"""
    data = rng.integers(48, 58, (n, LEN), dtype=np.uint8)
    data[:, 0] = rng.integers(49, 57, n, dtype=np.uint8)
    head = np.array([int(bytes(r)) for r in data[:1000]], np.int64)
    return np.full(n, LEN, np.int32), data.reshape(-1), head


def best_of(ctx, fn, reps=5):
    fn()                                        # warm-up: compiles, allocates
    out = []
    for _ in range(reps):
        ctx.synchronize()
        ctx.timer_start()
        fn()
        out.append(ctx.timer_stop())
    return min(out), out


def kernel_ms(ctx, fn, names):
    ctx.profile(True)
    before = {k: ctx.profile_get(k) for k in names}
    fn()
    got = {k: ctx.profile_get(k) for k in names}
    ctx.profile(False)
    return {k: (v[0] - before[k][0], v[1] - before[k][1]) for k, v in got.items() if v[0] > before[k][0]}


def line(name, ms, rows, bytes_per_row):
    gbps = rows * bytes_per_row / ms / 1e6
    print(f"{name:<58s} {ms:9.3f} ms  {rows / ms / 1e3:9.1f} MRows/s  {gbps:8.1f} GB/s  {100 * gbps / PEAK_GBPS:5.1f} % of peak")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import dfdb
    from dfdb import _native as N
    from dfdb import ir
    n = a.rows
    ctx = dfdb.default_context(0)
    sizes, data, head = build_column(n, np.random.default_rng(1))
    t = dfdb.DFTable.new(block_size=65536)
    N.check(N.load().dfdb_table_add_column(t._h, b"s", ir.STRING, n, sizes.ctypes.data, data.ctypes.data, len(data), None))
    t.add_column("k", np.arange(n, dtype=np.int64))
    probe = bytes(data[:LEN]).decode()
    del data, sizes
    print(f"# {ctx.device_info()['name']}: {n} rows of {LEN}-digit strings, block size 65536; best of 5 after a warm-up, HIP events")
    bpr = 4 + LEN + 8
    names = ["str_parse", "jit_project", "interp_project", "jit_predicate", "interp_predicate", "str_match", "gather"]
    added = [0]

    def parsed(extra=None):
        return dfdb.DFView(t)[dfdb.ALL, {"r": ("s", (lambda s: ir.parse(ir.I64, s)) if extra is None else extra)}]

    def add(extra=None):
        added[0] += 1
        t.add_column_from(f"id{added[0]}", parsed(extra))

    for knob, jit, label in ((1, 2, "conversion kernel"), (0, 2, "interpreter form, run-time compiled"), (0, 0, "interpreter form, interpreted")):
        ctx.set_option("parse_kernel", knob)
        ctx.set_option("jit", jit)
        ctx.set_option("jit_min_rows", 0)
        ms, _ = best_of(ctx, add)
        line(f"add_column_from(parse(I64, s)), {label}", ms, n, bpr)
        for k, (cnt, kms) in kernel_ms(ctx, add, names).items():
            line(f"  kernel {k} x{cnt}", kms, n, bpr)
    ctx.set_option("parse_kernel", 1)
    got = dfdb.materialize(dfdb.DFView(t)[dfdb.jr(1, 1000), dfdb.ALL][dfdb.ALL, ["id1"]])["id1"].to_numpy()
    assert np.array_equal(got, head), "the parsed column differs from int(s)"

    ctx.set_option("jit", 2)
    sel = dfdb.DFView(t)[ir.col(1) % 10 == 3, dfdb.ALL]

    def mat():
        v = sel[dfdb.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s))}]
        v._query().execute()
        return v

    def timed_mat():
        v = mat()
        ctx.synchronize()
        ctx.timer_start()
        r = dfdb.materialize(v)["r"].to_numpy()
        ms = ctx.timer_stop()
        assert len(r) == n // 10
        return ms
    timed_mat()
    ms = min(timed_mat() for _ in range(5))
    line("materialize(parse(I64, s)) at 10 % selected, to the host", ms, n // 10, bpr)
    for k, (cnt, kms) in kernel_ms(ctx, lambda: dfdb.materialize(mat()), names).items():
        if k in ("str_parse", "jit_project", "interp_project"):
            line(f"  kernel {k} x{cnt} (reads every selected tile)", kms, n // 10, bpr)

    def eq():
        return dfdb.DFView(t)[ir.col(0) == probe, dfdb.ALL]._query().count()
    ms, _ = best_of(ctx, eq)
    line(f"yardstick: count(s == \"{probe}\")", ms, n, 4 + LEN)
    for k, (cnt, kms) in kernel_ms(ctx, eq, names).items():
        line(f"  kernel {k} x{cnt}", kms, n, 4 + LEN)
    print("# the tutorial's figure for the same conversion: 109.95 MRows at 7.81 MRows/s, which includes a disk write on one CPU core")


if __name__ == "__main__":
    main()
