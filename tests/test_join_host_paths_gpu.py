"""What the host side of csrc/join.cpp launches, pinned: dfdb_query_join and dfdb_query_join_n each counted per call with the context's profile, and their
answers — npairs, every word of info, both fetched lists, for all four kinds — compared with tests/join_cases.py (one key) and tests/join_n_cases.py (several).
The counts are LaunchTimer scopes (the two scans of a count phase are one "scan_counts"; a scope whose launcher finds nothing to launch still counts) and
follow from the code.  With P = the digit passes the right side's sort runs (info[4]; every pass is one sort_count, one scan_counts, one sort_scatter):

  the left side, when it has a row (both entry points): sort_rows 1, and after the match step scan_counts 1 over the group totals.  No left row: nothing.
  the fetch: join_expand 1 when there is a pair, nothing otherwise.

  A  dfdb_query_join, Int64 nullable on both sides.  The right side is the sort's build and passes: a nullable build counts first, so sort_build 2 and one
     scan_counts, then P passes.  Then ONE join_probe.  scan_counts = 1 + P + 1.  No live walk, no refine, no rekey, no order laid.
  B  the same columns through dfdb_query_join_n with one key.  The right side is the sort driver with a sink: the same build and passes, and the sink's order
     laid (sort_order 1).  The right key is nullable: join_live count, scan_counts, join_live place.  The left side starts with join_live (start); one stage:
     sort_rekey 1 over the right order, join_refine 1 = join_refine.1.  scan_counts = 1 + P + 1 + 1.  No probe.  info[:5] is A's, info[5] = 1.
  C  dfdb_query_join_n on (i, s, s) against (i, s, s): i Int64 nullable, s String nullable, the longest live string 10 bytes (m = 2).
     The sort driver, most minor key first — s: str_row_offsets 1, sort_rows 1 (no order yet), then per sub-key (length, chunk 1, chunk 0) a count launch
     ("sort_strkey"), scan_counts and the write launch ("sort_strkey_len" for the length, "sort_strkey" for a chunk), an order laid before each chunk
     (sort_order 2); s again: the same with an order laid before the length too (sort_order 3) and offsets of its own (str_row_offsets 1); i: sort_order 1,
     sort_rekey 2 (count, write), scan_counts 1; the sink's order: sort_order 1.  So far str_row_offsets 2, sort_rows 1, sort_order 7, sort_strkey 10,
     sort_strkey_len 2, sort_rekey 2, scan_counts 7 + P.
     The join — right live walk: join_live 2, scan_counts 1; left: sort_rows 1, join_live 1; seven stages (i; s: chunk 0, chunk 1, length; s again):
     sort_rekey 1, sort_strkey 4, sort_strkey_len 2, join_refine 7 = join_refine.1 .. .7, and the LEFT column's offsets built once for both positions:
     str_row_offsets 1; scan_counts 1.
     Together: str_row_offsets 3, sort_rows 2, sort_order 7, sort_strkey 14, sort_strkey_len 4, sort_rekey 3, scan_counts 9 + P, join_live 3, join_refine 7.
  D  an empty selection.  Empty RIGHT side: its sort ends before any launch (both entry points), nr = 0.  dfdb_query_join still makes its one join_probe
     over the left rows (every search of an empty right side finds nothing): sort_rows 1, join_probe 1, scan_counts 1.  dfdb_query_join_n: no live walk on
     the right (no row), no stage (info[5] = 0): sort_rows 1, join_live 1 (start, which emits what cnt = 0 emits), scan_counts 1.  The totals are 0 / nl / 0 / nl.
     Empty LEFT side: the right side is built as in A / B (B without the stage: join_live 2), nothing else is launched, the totals are 0 and nothing is fetched.
     Both empty: no launch at all.
  E  a refused call (a type mismatch) launches nothing, touches no output and drops the pending join; the next good call launches what A / B launch."""
import numpy as np
import pytest

import join_cases as J
import join_n_cases as JN
from test_join_gpu import add_raw, counted, raw_join
from test_join_n_gpu import SENTINEL, raw_join_n

pytestmark = pytest.mark.gpu

NL, NR = 5000, 3000                                         # five and three 1024-entry groups, the last one partial
STAGES = tuple(f"join_refine.{k}" for k in range(1, 9)) + ("join_refine.9+",)
NAMES = ("join_probe", "join_refine", "join_live", "join_expand", "sort_rows", "sort_rekey", "sort_strkey", "sort_strkey_len", "str_row_offsets", "scan_counts",
         "sort_build", "sort_order", "sort_count", "sort_scatter", "sort_emit") + STAGES
PROJ = ["i", "s", "f"]


def launches(passes=0, scan_counts=0, join_refine=0, **named):
    """every name of NAMES at 0, but: the three launches of each of the P passes, the scans beside the passes', one refine per stage, and what the case names"""
    c = dict.fromkeys(NAMES, 0)
    c.update(sort_count=passes, sort_scatter=passes, scan_counts=passes + scan_counts, join_refine=join_refine, **named)
    c.update({STAGES[k]: 1 for k in range(join_refine)})
    assert set(c) == set(NAMES)
    return c


class Side:
    """a table with i (Int64, nullable), s (String, nullable; 10 and 9 bytes), f (Float64) and u (the row number, for a predicate that selects nothing)"""

    def __init__(self, dfdb, ctx, n, every_i, every_s, seed):
        self.n = n
        self.i = (np.arange(n) % 600).astype(np.int64)      # two key bytes vary: the sort runs digit passes
        self.imiss = np.arange(n) % every_i == every_i - 1
        pool = [b"abcdefghi" + bytes([97 + j]) for j in range(5)] + [b"abcdefgh" + bytes([97 + j]) for j in range(5)]
        draw = np.random.default_rng([n, seed]).integers(0, 10, n)
        self.s = JN.with_missing([pool[k] for k in draw], np.arange(n) % every_s == 3)
        self.t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
        add_raw(dfdb, self.t, "i", self.i, self.imiss)
        self.t.add_column("s", self.s)
        add_raw(dfdb, self.t, "f", self.i.astype(np.float64))
        add_raw(dfdb, self.t, "u", np.arange(n, dtype=np.int64))
        self.all = self.t[dfdb.ALL, PROJ]._query()
        self.none = self.t[("u", lambda u: u < 0), PROJ]._query()
        assert (self.all.count(), self.none.count()) == (n, 0)      # both selections are executed here: the counted calls scan nothing

    def comps(self, cols):
        return [((self.i, self.imiss), (self.s, None))[c] for c in cols]


@pytest.fixture(scope="module")
def sides(dfdb_mod, ctx):
    left, right = Side(dfdb_mod, ctx, NL, 7, 11, 1), Side(dfdb_mod, ctx, NR, 5, 13, 2)
    assert JN.chunks_of(right.s) == 2
    yield left, right
    left.t.close()
    right.t.close()


def check_kinds(ctx, ql, call, want, expect, info5=None, case=None):
    """call(kind code) -> (npairs, info) and the fetch, counted apart, for all four kinds; expect(info) -> the launches of call 1.  Returns kind -> info"""
    infos = {}
    for kind in J.KINDS:
        wl, wr, winfo = want[kind]
        (n, info), c = counted(ctx, NAMES, lambda: call(J.KIND_CODE[kind]))
        assert n == len(wl) and info[:4] == winfo, (case, kind, n, len(wl), info, winfo)
        assert len(info) == (5 if info5 is None else 6) and (info5 is None or info[5] == info5), (case, kind, info)
        assert c == expect(info), (case, kind, info, c)
        (gl, gr), c = counted(ctx, NAMES, lambda: ql.join_fetch(n))
        assert c == launches(join_expand=1 if n else 0), (case, kind, c)
        assert gl.dtype == np.int64 and np.array_equal(gl, wl) and np.array_equal(gr, wr), (case, kind, gl[:8], wl[:8], gr[:8], wr[:8])
        infos[kind] = info
    return infos


def one_key_want(left, right, lrows=None, rrows=None):
    return J.join_ref_all(left.i, left.imiss, lrows, right.i, right.imiss, rrows)


def launches_a(info):
    return launches(info[4], sort_build=2, scan_counts=2, sort_rows=1, join_probe=1)


def launches_b(info):
    return launches(info[4], sort_build=2, sort_order=1, scan_counts=3, join_live=3, sort_rows=1, sort_rekey=1, join_refine=1)


def test_one_nullable_key_through_both_entry_points(dfdb_mod, ctx, sides):
    """cases A and B"""
    left, right = sides
    ql, qr = left.all, right.all
    want = one_key_want(left, right)
    assert want["inner"][2] == (NL, NR, int(left.imiss.sum()), int(right.imiss.sum())) and len(want["inner"][0]) > NL
    passes = qr.sort_indices(0, False, None)[1][2]          # what the sort itself reports for the same key
    a = check_kinds(ctx, ql, lambda kind: ql.join_count(qr, 0, 0, kind), want, launches_a, case="A")
    b = check_kinds(ctx, ql, lambda kind: ql.join_count_n(qr, [0], [0], kind), want, launches_b, info5=1, case="B")
    for kind in J.KINDS:
        assert a[kind][4] == passes and b[kind][:5] == a[kind], (kind, passes, a[kind], b[kind])


def test_a_string_column_in_two_key_positions(dfdb_mod, ctx, sides):
    """case C"""
    left, right = sides
    ql, qr = left.all, right.all
    cols = [0, 1, 1]
    want = JN.join_n_ref_all(left.comps(cols), None, right.comps(cols), None)
    assert 0 < len(want["inner"][0]) and want["inner"][2][2] > int(left.imiss.sum()) and want["inner"][2][3] > int(right.imiss.sum())
    passes = qr.sort_indices_any(cols)[1][2]

    def expect(info):
        return launches(info[4], str_row_offsets=3, sort_rows=2, sort_order=7, sort_strkey=14, sort_strkey_len=4, sort_rekey=3, scan_counts=9, join_live=3, join_refine=7)

    c = check_kinds(ctx, ql, lambda kind: ql.join_count_n(qr, cols, cols, kind), want, expect, info5=7, case="C")
    assert all(c[kind][4] == passes for kind in J.KINDS), (passes, c)


def test_an_empty_selection_on_either_side(dfdb_mod, ctx, sides):
    """case D"""
    left, right = sides
    none_l, none_r = np.zeros(0, np.int64), np.zeros(0, np.int64)
    # no right row
    ql, qr = left.all, right.none
    want = one_key_want(left, right, rrows=none_r)
    assert [len(want[k][0]) for k in J.KINDS] == [0, NL, 0, NL]
    a = check_kinds(ctx, ql, lambda kind: ql.join_count(qr, 0, 0, kind), want, lambda info: launches(sort_rows=1, join_probe=1, scan_counts=1), case="A, no right row")
    b = check_kinds(ctx, ql, lambda kind: ql.join_count_n(qr, [0], [0], kind), want, lambda info: launches(sort_rows=1, join_live=1, scan_counts=1), info5=0,
                    case="B, no right row")
    assert all(a[k] == (NL, 0, int(left.imiss.sum()), 0, 0) and b[k] == a[k] + (0,) for k in J.KINDS), (a, b)
    # no left row
    ql, qr = left.none, right.all
    want = one_key_want(left, right, lrows=none_l)
    assert [len(want[k][0]) for k in J.KINDS] == [0, 0, 0, 0]
    a = check_kinds(ctx, ql, lambda kind: ql.join_count(qr, 0, 0, kind), want, lambda info: launches(info[4], sort_build=2, scan_counts=1), case="A, no left row")
    b = check_kinds(ctx, ql, lambda kind: ql.join_count_n(qr, [0], [0], kind), want,
                    lambda info: launches(info[4], sort_build=2, sort_order=1, scan_counts=2, join_live=2), info5=0, case="B, no left row")
    assert all(a[k][4] > 0 and a[k] == (0, NR, 0, int(right.imiss.sum()), a[k][4]) and b[k] == a[k] + (0,) for k in J.KINDS), (a, b)
    # neither
    ql, qr = left.none, right.none
    want = one_key_want(left, right, none_l, none_r)
    a = check_kinds(ctx, ql, lambda kind: ql.join_count(qr, 0, 0, kind), want, lambda info: launches(), case="A, no row")
    b = check_kinds(ctx, ql, lambda kind: ql.join_count_n(qr, [0, 1], [0, 1], kind), want, lambda info: launches(), info5=0, case="B, no row")
    assert all(a[k] == (0, 0, 0, 0, 0) and b[k] == (0, 0, 0, 0, 0, 0) for k in J.KINDS), (a, b)


def test_a_refusal_between_two_good_calls(dfdb_mod, ctx, sides):
    """case E"""
    from dfdb import _native as N
    left, right = sides
    ql, qr = left.all, right.all
    want = one_key_want(left, right)
    wl, wr, _ = want["left"]
    for good, refused, pattern, absent, expect in (
            (lambda: ql.join_count(qr, 0, 0, dfdb_mod.JOIN_LEFT), lambda: raw_join(ql, qr, 0, 2, 0), "different types (Int64 and Float64)", "key ", launches_a),
            (lambda: ql.join_count_n(qr, [0], [0], dfdb_mod.JOIN_LEFT), lambda: raw_join_n(ql, qr, [0, 0], [0, 2], 0), "different types (key 1: Int64 and Float64)", None, launches_b)):
        n, _ = good()
        assert n == len(wl)
        (rc, npairs, info), c = counted(ctx, NAMES, refused)                                # while that join is pending
        assert rc == N.ERR_UNSUPPORTED and pattern in N.last_error() and (absent is None or absent not in N.last_error()), (rc, N.last_error())
        assert npairs == SENTINEL and np.all(info == SENTINEL) and c == launches(), (npairs, info, c)
        with pytest.raises(ValueError, match="has not been called"):
            ql.join_fetch(n)
        (n, info), c = counted(ctx, NAMES, good)                                            # and the next good call works
        assert n == len(wl) and info[:4] == want["left"][2] and c == expect(info), (n, info, c)
        gl, gr = ql.join_fetch(n)
        assert np.array_equal(gl, wl) and np.array_equal(gr, wr)
