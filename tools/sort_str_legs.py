#!/usr/bin/env python3
"""Legs of dfdb_sort_indices_any over a String key (csrc/sort.cpp, k_sort_strkey of csrc/k_sort.hip: a String key run as its m + 1 eight-byte sub-keys —
length, then chunk m-1 .. chunk 0 — through the one sort driver), measured on one GPU.

Input: config 4's strings — --rows (default 5e8) resident rows of the ten-brand generator — under a selection that keeps one row in five (1e8 rows), beside
m + 1 Int64 columns of ten values each (m is what the String call reports: info[2] + info[3] = 8 (m + 1)).  On an EXECUTED query every round times,
interleaved, whole calls into device memory:

  (s)  dfdb_sort_indices_any by the String column
  (y)  dfdb_sort_indices_n by the m + 1 Int64 columns: the YARDSTICK — the existing path doing the same number of sub-sorts over the same selection (its most
       minor key is built from the bitmap, the others by k_sort_rekey: one gather per entry where the String key has two or three)

and, from one more (s) call with the context's per-launch profiling on, what its launches took: the offsets build (k_str_row_offsets, once per key), the
length's k_sort_strkey launch (profile name sort_strkey_len: the sizes-only build — it loads no offset and no arena byte), the chunks' launches (sort_strkey)
and the passes.  The sizes-only cost the line prints is the offsets build + the length's launch.  No threshold is fixed in advance: the line
prints (s) / (y).  The time is expected to be bound by 128-byte lines per gathered entry, as the rekey's is: the size, the in-tile offset and the arena line
per chunk.

  (h)  --host-rounds times (default 1: it takes minutes and gigabytes): materialize the selection's strings to the host and sorted() over (bytes, row) —
       what a caller does without the entry point; its row order must equal the device's

(s), (y) are timed with HIP events around the whole call, (h) with the host clock.  ROUNDS rounds after a warm-up; the figure is the median, the spread is
max - min.

    python tools/sort_str_legs.py > profiles/sort_str.txt
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000_000)
    ap.add_argument("--host-rounds", type=int, default=1)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import dfdb
    ctx = dfdb.default_context(0)
    dev = torch.device("cuda", 0)
    n = a.rows
    t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    t.add_generated("s", dfdb.GEN_STR_BRANDS10, 4, n)
    t.add_generated("u", dfdb.GEN_I64_MOD1M, 13, n)
    t.add_column_from("u5", t[dfdb.ALL, ("u", lambda u: u % 5)])
    sel = ("u5", lambda u: u < 1)
    qs = t[sel, ["s"]]._query()
    cnt = qs.count()                                                   # executes the selection: the bitmap stays
    out = torch.empty(max(cnt, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    info = {}

    def string_key():
        info["s"] = qs.sort_indices_any([0], None, None, dev_ptr=out.data_ptr(), cap=cnt)[1]

    string_key()
    ctx.synchronize()
    nsub = (info["s"][2] + info["s"][3]) // 8                          # m + 1
    names = []
    for j in range(nsub):                                              # the yardstick's keys: ten values each, like the brands
        t.add_generated(f"g{j}", dfdb.GEN_I64_MOD1M, 21 + j, n)
        t.add_column_from(f"k{j}", t[dfdb.ALL, (f"g{j}", lambda g: g % 10)])
        names.append(f"k{j}")
    qy = t[sel, names]._query()
    assert qy.count() == cnt

    def yardstick():
        info["y"] = qy.sort_indices_n(list(range(nsub)), None, None, dev_ptr=out.data_ptr(), cap=cnt)[1]

    def timed(f):
        ctx.synchronize(); ctx.timer_start(); f(); return ctx.timer_stop()

    print(f"# {ctx.device_info()['name']}: dfdb_sort_indices_any by a String column into device memory, {n} resident rows (ten brands), {cnt} rows selected, "
          f"m + 1 = {nsub} sub-keys; whole calls on an executed query, HIP events, {ROUNDS} interleaved rounds after a warm-up (median, spread = max - min); every "
          f"figure measured on this one GPU", flush=True)
    for f in (string_key, yardstick):
        f(); f()
    ms = {"s": [], "y": []}
    for _ in range(ROUNDS):
        ms["y"].append(timed(yardstick)); ms["s"].append(timed(string_key))
    s, y = med(ms["s"]), med(ms["y"])
    print(f"(s) String key         n {cnt:>10d}  {s:9.3f} ms (spread {spread(ms['s']):7.3f}; pairs {info['s'][1]}, passes {info['s'][2]} run {info['s'][3]} skipped)", flush=True)
    print(f"(y) {nsub} Int64 keys (_n)   n {cnt:>10d}  {y:9.3f} ms (spread {spread(ms['y']):7.3f}; pairs {info['y'][1]}, passes {info['y'][2]} run {info['y'][3]} skipped)  "
          f"(s) / (y) = {s / y:5.2f}", flush=True)
    parts = ("str_row_offsets", "sort_rows", "sort_strkey_len", "sort_strkey", "sort_order", "sort_count", "sort_scatter", "scan_counts", "sort_emit")
    ctx.synchronize(); ctx.profile(True); string_key(); ctx.synchronize()
    prof = {k: ctx.profile_get(k) for k in parts}
    ctx.profile(False)
    nk, kms = prof["sort_strkey"]
    lms, oms = prof["sort_strkey_len"][1], prof["str_row_offsets"][1]
    print("(s) one profiled call: " + ", ".join(f"{k} {prof[k][1]:.3f} ms ({prof[k][0]})" for k in parts) +
          f"; a chunk's k_sort_strkey launch: {kms / max(nk, 1):.3f} ms = {cnt / max(kms / max(nk, 1), 1e-9) / 1e6:6.1f} G entries/s; the length's: {lms:.3f} ms = "
          f"{cnt / max(lms, 1e-9) / 1e6:6.1f} G entries/s; sizes-only cost (offsets build + the length's launch): {oms + lms:.3f} ms", flush=True)
    if not a.host_rounds:
        print("(h) host materialize + sorted: not measured in this run (--host-rounds 0)", flush=True)
        return
    string_key()
    ctx.synchronize()
    got = out[:cnt].cpu().numpy()
    host = []
    for _ in range(a.host_rounds):
        t0 = time.perf_counter()
        sizes, data = t[sel, ["s"]]._query().materialize()[0]          # (a query of its own: the scan is part of what the host path costs)
        ends = np.cumsum(sizes.clip(min=0), dtype=np.int64)
        raw = data.tobytes()
        strs = [raw[e - z:e] for e, z in zip(ends.tolist(), sizes.tolist())]
        order = sorted(range(len(strs)), key=strs.__getitem__)        # (stable: ties in ascending row order)
        host.append((time.perf_counter() - t0) * 1e3)
    rows = qs.indices()[np.asarray(order, np.int64)]
    assert np.array_equal(got, rows), (got[:8], rows[:8])
    h = med(host)
    print(f"(h) host materialize + sorted over bytes  n {cnt:>10d}  {h:10.1f} ms (spread {spread(host):9.1f}) = {h / s:7.1f} x (s); the two row orders are equal", flush=True)


if __name__ == "__main__":
    main()
