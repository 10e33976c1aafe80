#!/usr/bin/env python3
"""Legs of dfdb_gather_rows_any over a String column (csrc/sort.cpp, csrc/k_str_rows.hip: sizes pass, scan, bytes pass), measured on one GPU.

Input: config 4's strings — --rows (default 5e8) resident rows of the ten-brand generator beside an Int64 key — under a selection that keeps one row in five
(1e8 rows).  On an EXECUTED query every round times, interleaved, whole calls into device memory (rows, sizes and bytes all stay on the device; the bytes
buffers are sized once, before the rounds, as dfdb_gather_rows_string_bytes / dfdb_result_string_bytes size them):

  (asc)  dfdb_gather_rows_any, rows = the selection's rows ascending (dfdb_select_indices into device memory)
  (ord)  dfdb_gather_rows_any, rows = the same rows in the order of the Int64 key (dfdb_sort_indices into device memory)
  (k6)   dfdb_materialize of the same column over the same selection: K6, the yardstick of (asc) — same bytes out, coalesced source
  (lay)  dfdb_gather_rows_string_bytes over the ascending rows: the layout call alone

Expectations recorded and judged: (asc) lies within the two spreads combined of (k6) + the offsets build (k_str_row_offsets, from one profiled call: K6 needs
no per-row offset array); (ord) is bound by 128-byte lines, as k_sort_rekey is: every output pulls a line of sizes, a line of row offsets and one or two of
the arena for a handful of bytes — the line says what that comes to per output.

  (top)  the first 10 rows of (ord)'s order, in each form of the in-tile prefix (ctx option "str_gather_form": 1 offsets, 2 direct)
  (x)    the first n rows of (ord)'s order for n = rows/2048, /1024, /512, /256, /128, in each form: where the two forms cross.  The rule (kernels.hpp:
         str_gather_form) says direct when n * 512 <= rows, from the bytes the forms move; if the measured crossover lies more than 2x away the constant moves
  (h)    --host-rounds times (default 1: it takes a minute and gigabytes): materialize the selection's strings to the host and take them from the Python
         list in key order — what a caller did before the entry point; a sample of its strings must equal the device's

HIP events around the whole call ((h): the host clock), ROUNDS rounds after a warm-up; the figure is the median, the spread is max - min.

    python tools/str_gather_rows_legs.py > profiles/str_gather_rows.txt
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
FORMS = {1: "offsets", 2: "direct"}


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
    from dfdb import _native as N
    ctx = dfdb.default_context(0)
    L = N.load()
    dev = torch.device("cuda", 0)
    n = a.rows
    t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    t.add_generated("s", dfdb.GEN_STR_BRANDS10, 4, n)
    t.add_generated("a", dfdb.GEN_I64_MOD1M, 5, n)
    t.add_generated("u", dfdb.GEN_I64_MOD1M, 13, n)
    t.add_column_from("u5", t[dfdb.ALL, ("u", lambda u: u % 5)])
    sel = ("u5", lambda u: u < 1)
    q = t[sel, ["s"]]._query()
    cnt = q.count()                                                    # executes the selection: the bitmap stays
    asc = torch.empty(max(cnt, 1), dtype=torch.int64, device=dev)
    order = torch.empty(max(cnt, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    q.indices_device(asc.data_ptr(), cnt)
    t[sel, ["a"]]._query().sort_indices(0, False, None, dev_ptr=order.data_ptr(), cap=cnt)
    ctx.synchronize()
    nb = C.c_int64()
    N.check(L.dfdb_result_string_bytes(q._h, 0, C.byref(nb)))
    assert nb.value == q.gather_rows_string_bytes(0, dev_ptr=asc.data_ptr(), n=cnt) == q.gather_rows_string_bytes(0, dev_ptr=order.data_ptr(), n=cnt)
    sizes = torch.empty(max(cnt, 1), dtype=torch.int32, device=dev)
    data = torch.empty(nb.value + 64, dtype=torch.uint8, device=dev)
    outs = (N.OutCol * 1)()
    outs[0].data, outs[0].bytes, outs[0].bytes_cap, outs[0].memkind = sizes.data_ptr(), data.data_ptr(), nb.value, N.MEM_DEVICE
    torch.cuda.synchronize()
    print(f"# {ctx.device_info()['name']}: dfdb_gather_rows_any of a String column into device memory, {n} resident rows (ten brands), {cnt} rows selected, "
          f"{nb.value} string bytes out; whole calls on an executed query, HIP events, {ROUNDS} interleaved rounds after a warm-up (median, spread = max - min); "
          f"every figure measured on this one GPU", flush=True)

    def gather(rows, m, form=0):
        ctx.set_option("str_gather_form", form)
        N.check(L.dfdb_gather_rows_any(q._h, C.c_void_p(rows.data_ptr()), m, N.MEM_DEVICE, outs, 1))
        ctx.set_option("str_gather_form", 0)

    def k6():
        N.check(L.dfdb_materialize(q._h, outs, 1))

    def layout():
        N.check(L.dfdb_gather_rows_string_bytes(q._h, 0, C.c_void_p(asc.data_ptr()), cnt, N.MEM_DEVICE, C.byref(nb)))

    def timed(f):
        ctx.synchronize(); ctx.timer_start(); f(); return ctx.timer_stop()

    def rounds(legs):
        for f in legs.values():
            f(); f()
        ms = {k: [] for k in legs}
        for _ in range(ROUNDS):
            for k, f in legs.items():
                ms[k].append(timed(f))
        return ms

    def profiled(f, names):
        ctx.synchronize(); ctx.profile(True); f(); ctx.synchronize()
        got = {k: ctx.profile_get(k) for k in names}
        ctx.profile(False)
        return got

    # ---- the whole selection, ascending and in key order, against K6
    k6()
    ctx.synchronize()
    want_sizes, want_bytes = sizes.clone(), data[:nb.value].clone()
    gather(asc, cnt)
    ctx.synchronize()
    assert torch.equal(sizes, want_sizes) and torch.equal(data[:nb.value], want_bytes), "the ascending gather differs from dfdb_materialize"
    ms = rounds({"asc": lambda: gather(asc, cnt), "k6": k6, "ord": lambda: gather(order, cnt), "lay": layout})
    parts = ("str_row_offsets", "str_rows_sizes", "scan_counts", "str_rows_bytes")
    pa, po = profiled(lambda: gather(asc, cnt), parts), profiled(lambda: gather(order, cnt), parts)
    build = pa["str_row_offsets"][1]
    m_asc, m_k6, m_ord = med(ms["asc"]), med(ms["k6"]), med(ms["ord"])
    both = spread(ms["asc"]) + spread(ms["k6"])
    diff = m_asc - (m_k6 + build)
    verdict = "WITHIN the two spreads combined of that" if abs(diff) <= both else ("BELOW that by more than the two spreads combined" if diff < 0 else
                                                                                   "ABOVE that by more than the two spreads combined")
    print(f"(asc) ascending rows   n {cnt:>10d}  {m_asc:9.3f} ms (spread {spread(ms['asc']):7.3f})  one profiled call: " +
          ", ".join(f"{k} {pa[k][1]:.3f} ms ({pa[k][0]})" for k in parts), flush=True)
    print(f"(k6)  dfdb_materialize n {cnt:>10d}  {m_k6:9.3f} ms (spread {spread(ms['k6']):7.3f})  (k6) + offsets build = {m_k6 + build:9.3f} ms; (asc) is "
          f"{verdict} ({diff:+.3f} ms against {both:.3f}; (asc) / (k6) = {m_asc / m_k6:5.2f})", flush=True)
    print(f"(ord) rows in key order n {cnt:>10d}  {m_ord:9.3f} ms (spread {spread(ms['ord']):7.3f}) = {m_ord * 1e6 / max(cnt, 1):6.3f} ns per output, (ord) / (asc) = "
          f"{m_ord / m_asc:5.2f}; one profiled call: " + ", ".join(f"{k} {po[k][1]:.3f} ms" for k in parts) +
          f"; the sizes pass pulls two 128-byte lines per output (a size, a row offset) = {2 * 128 * cnt / max(po['str_rows_sizes'][1], 1e-9) / 1e6:7.1f} GB/s of lines, "
          f"the bytes pass one or two = {128 * cnt / max(po['str_rows_bytes'][1], 1e-9) / 1e6:7.1f} to {2 * 128 * cnt / max(po['str_rows_bytes'][1], 1e-9) / 1e6:7.1f} GB/s", flush=True)
    print(f"(lay) dfdb_gather_rows_string_bytes, ascending rows  {med(ms['lay']):9.3f} ms (spread {spread(ms['lay']):7.3f})", flush=True)

    # ---- few rows of a long column: the two forms
    def forms_at(label, m):
        legs = {FORMS[f]: (lambda f=f: gather(order, m, f)) for f in FORMS}
        r = rounds(legs)
        o, d = med(r["offsets"]), med(r["direct"])
        rule = "direct" if m * 512 <= n else "offsets"
        print(f"{label} n {m:>10d} (rows / {n / max(m, 1):9.1f})  offsets {o:9.3f} ms (spread {spread(r['offsets']):7.3f})  direct {d:9.3f} ms (spread {spread(r['direct']):7.3f})  "
              f"the faster: {'direct' if d < o else 'offsets'} by {max(o, d) / max(min(o, d), 1e-9):6.2f} x; the rule takes {rule}", flush=True)
        return o, d

    forms_at("(top) limit = 10    ", min(10, cnt))
    xs = [(k, min(n // k, cnt)) for k in (2048, 1024, 512, 256, 128)]
    res = [(k, m) + forms_at(f"(x)   rows / {k:<5d}", m) for k, m in xs]
    faster = ["direct" if d < o else "offsets" for _, _, o, d in res]
    said = " / ".join(f"{f} at rows / {k}" for (k, _, _, _), f in zip(res, faster))
    flips = [i for i in range(1, len(res)) if faster[i - 1] == "direct" and faster[i] == "offsets"]
    if len(flips) == 1 and faster[:flips[0]] == ["direct"] * flips[0] and faster[flips[0]:] == ["offsets"] * (len(res) - flips[0]):
        # between the two points that bracket it both forms are close to straight lines in n: where the lines meet
        (_, m0, o0, d0), (_, m1, o1, d1) = res[flips[0] - 1], res[flips[0]]
        x = m0 + (m1 - m0) * (o0 - d0) / ((o0 - d0) - (o1 - d1))
        ratio = n / x
        away = max(ratio / 512, 512 / ratio)
        verdict = (f"the forms cross at n = {x:,.0f} = rows / {ratio:.0f} (the two bracketing points joined by straight lines), {away:.2f} x away from the rule's "
                   f"n = rows / 512: {'MORE than 2 x, the constant moves' if away > 2 else 'within 2 x, the constant derived from the bytes stays'}")
    elif faster == ["direct"] * len(res):
        verdict = "direct is the faster form up to rows / 128 at least: the measured crossover lies MORE than 2 x above n = rows / 512"
    elif faster == ["offsets"] * len(res):
        verdict = "offsets is the faster form from rows / 2048 on: the measured crossover lies MORE than 2 x below n = rows / 512"
    else:
        verdict = "the faster form changes more than once over these points: no crossover can be read from them"
    print(f"(x)   crossover: {said} — {verdict}", flush=True)

    # ---- the host path the entry point replaces
    if a.host_rounds:
        gather(order, cnt)
        ctx.synchronize()
        k = min(cnt, 1000)
        hs, ho = sizes[:k].cpu().numpy(), data.cpu().numpy()
        dev_head = dfdb.api._flat_to_strings(hs, ho[:int(np.maximum(hs, 0).sum())])
        perm = np.searchsorted(asc.cpu().numpy(), order.cpu().numpy())  # where every row of the key order stands among the selected rows
        host = []
        for _ in range(a.host_rounds):
            t0 = time.perf_counter()
            col = dfdb.materialize(t[sel, "s"])                        # the selection's strings to the host, as Python strings
            taken = [col[i] for i in perm]                             # take on the list
            host.append((time.perf_counter() - t0) * 1e3)
            assert list(taken[:k]) == dev_head, "the host's take differs from the device's"
            del col, taken
        h = med(host)
        print(f"(h)   host materialize of the selection ({cnt} strings) + take from the list in key order  {h:12.1f} ms (spread {spread(host):9.1f}, {a.host_rounds} round(s)) = "
              f"{h / m_ord:8.1f} x (ord); its first {k} strings equal the device's", flush=True)
    else:
        print("(h)   host materialize + take: not measured", flush=True)
    t.close()


if __name__ == "__main__":
    main()
