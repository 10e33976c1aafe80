#!/usr/bin/env python3
"""Legs of `s1 OP s2` over two String columns, measured on one GPU.

Input: two String columns of config 4's shape made on the device (the brands10 generator: ten values of 4..9 bytes, mean 5.4, drawn per row from two
seeds, so the columns are equal in one row out of ten), at --rows (default 1e8 and 5e8).  Every form answers `count(s1 OP s2)` for == and <:

  (a) k_str_pair
  (b) the interpreter's H_STRCMP2 in the same build (str_pair_kernel = 0): compiled at run time (jit = 2) and interpreted (jit = 0)
  (c) K5's `s1 == "samsung"` over one of the columns: the ceiling for a scan that reads sizes and bytes (the pair kernel reads two such columns)
  (d) both columns with a dictionary: k_dict_pair, against the dictionary scan of one column

A whole count call is timed with HIP events on the engine stream (the kernel, the tile-count scan and the copy of the total); the forms are interleaved
round by round, ROUNDS rounds after a warm-up of every form; the figure is the median, the spread is min..max.  The kernels' own times come from the
per-launch profile of one more pass.  GB/s counts the bytes a form has to read (4 B of size + the string bytes per row and column; 2 B per code).

    python tools/str_pair_legs.py > profiles/str_pair.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dataframedbs.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ROUNDS = 9
MEAN_LEN = 5.4
PEAK_GBPS = 8000.0
KNOBS = {"str_pair_kernel": 1, "jit": 2}
NAMES = ["str_pair", "dict_pair", "dict_scan", "str_match", "jit_predicate", "interp_predicate", "scan_counts"]


def run_size(dfdb, ir, ctx, n):
    t = dfdb.DFTable.new(block_size=65536)
    t.add_generated("s1", dfdb.GEN_STR_BRANDS10, 11, n)
    t.add_generated("s2", dfdb.GEN_STR_BRANDS10, 12, n)
    pair_bytes, one_bytes = 2 * (4 + MEAN_LEN), 4 + MEAN_LEN

    def count(e):
        return dfdb.DFView(t)[e, dfdb.ALL]._query().count()

    def form(label, knobs, e, bpr):
        return {"label": label, "knobs": dict(KNOBS, **knobs), "e": e, "bpr": bpr, "ms": [], "count": None}

    def measure(forms, title):
        def run(f, timed):
            for k, v in f["knobs"].items():
                ctx.set_option(k, v)
            ctx.synchronize()
            if timed:
                ctx.timer_start()
            c = count(f["e"])
            if timed:
                f["ms"].append(ctx.timer_stop())
            assert f["count"] in (None, c), (f["label"], f["count"], c)
            f["count"] = c
        for f in forms:
            run(f, False); run(f, False)                                   # warm-up: compiles, allocates
        for _ in range(ROUNDS):
            for f in forms:                                                # interleaved: every round visits every form
                run(f, True)
        print(f"## {title}")
        for f in forms:
            ms = statistics.median(f["ms"])
            gbps = n * f["bpr"] / ms / 1e6
            ctx.profile(True)
            before = {k: ctx.profile_get(k) for k in NAMES}
            run(f, False)
            prof = {k: (ctx.profile_get(k)[0] - before[k][0], ctx.profile_get(k)[1] - before[k][1]) for k in NAMES}
            ctx.profile(False)
            kern = ", ".join(f"{k} {v[1]:.3f} ms" for k, v in prof.items() if v[0] > 0 and k != "scan_counts")
            print(f"{f['label']:<58s} median {ms:8.3f} ms  (min {min(f['ms']):8.3f}  max {max(f['ms']):8.3f})  {n / ms / 1e3:9.1f} MRows/s  {gbps:7.1f} GB/s "
                  f"{100 * gbps / PEAK_GBPS:5.1f} % of peak   count {f['count']}   kernel: {kern}")
        for k, v in KNOBS.items():
            ctx.set_option(k, v)

    s1, s2 = ir.col(0), ir.col(1)
    for name, e in (("==", s1 == s2), ("<", s1 < s2)):
        forms = [form(f"(a) k_str_pair: s1 {name} s2", {}, e, pair_bytes),
                 form(f"(b) interpreter form, run-time compiled: s1 {name} s2", {"str_pair_kernel": 0}, e, pair_bytes),
                 form(f"(b) interpreter form, interpreted: s1 {name} s2", {"str_pair_kernel": 0, "jit": 0}, e, pair_bytes),
                 form('(c) K5: s1 == "samsung"', {}, s1 == "samsung", one_bytes)]
        measure(forms, f"{n} rows, flat columns, s1 {name} s2")
        counts = {f["count"] for f in forms[:3]}
        assert len(counts) == 1, counts                                    # the three forms of one query agree
    assert t.build_dictionary("s1") == 10 and t.build_dictionary("s2") == 10
    forms = [form("(d) k_dict_pair: s1 == s2", {}, s1 == s2, 4), form("(d) k_dict_pair: s1 < s2", {}, s1 < s2, 4),
             form('(d) dictionary scan: s1 == "samsung"', {}, s1 == "samsung", 2)]
    measure(forms, f"{n} rows, both columns with a dictionary")
    t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[100_000_000, 500_000_000])
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import dfdb
    from dfdb import ir
    ctx = dfdb.default_context(0)
    ctx.set_option("jit_min_rows", 0)
    print(f"# {ctx.device_info()['name']}: count(s1 OP s2), brands10 columns (mean {MEAN_LEN} bytes, equal in 1 row of 10); whole count calls, HIP events, "
          f"{ROUNDS} interleaved rounds after a warm-up; every figure measured on this one GPU")
    for n in a.rows:
        run_size(dfdb, ir, ctx, n)


if __name__ == "__main__":
    main()
