"""dfdb_query_join_n (csrc/join.cpp over csrc/k_join.hip: the right side ordered by the key tuple through the sort driver, one k_join_refine launch per 8-byte
sub-key, one scan; the fetch is dfdb_query_join_fetch) against the restatement of tests/join_n_cases.py.  Every comparison is exact: both row lists, the number
of pairs, info[0:4] — and, after the calls, dfdb_count and dfdb_select_indices of both queries.  The sizes are the smallest at which each piece can go wrong:
row counts around a wave's round of 64 and a 1024-entry group, right sides around the powers of two a search steps through, runs that end at the last right
row, strings around the 8-byte chunk and at the 256-byte limit."""
import ctypes as C

import numpy as np
import pytest

import join_cases as J
import join_n_cases as JN
import order_stat_cases as K
from test_join_gpu import add_raw, counted, frame_equal, multiplicity_shapes

pytestmark = pytest.mark.gpu
SENTINEL = -7


def table_of(dfdb, ctx, comps, extra=()):
    """a table with key columns k0, k1, .. exactly as given (the bytes under a missing flag stay what they are) and further (name, values) columns"""
    t = dfdb.DFTable.new(block_size=65536, ctx=ctx)
    for j, (values, missing) in enumerate(comps):
        if JN.is_string(values):
            t.add_column(f"k{j}", [JN.as_bytes(v) for v in values])
        else:
            add_raw(dfdb, t, f"k{j}", values, missing)
    for name, values in extra:
        add_raw(dfdb, t, name, values)
    return t


def plain(*arrays):
    return [(a, None) for a in arrays]


def keys_view(dfdb, t, n, spec=None):
    names = [f"k{j}" for j in range(n)]
    if spec is None:
        return t[dfdb.ALL, names]
    if spec[0] == "range":
        return t[dfdb.jr(spec[1], spec[2], dfdb.END), names]
    if spec[0] == "indices":
        return t[list(spec[1]), names]
    k = spec[3]
    return t[(spec[1], (lambda c: c < k) if spec[2] == "<" else (lambda c: c == k)), names]


def check_views(vl, lcomps, vr, rcomps, lrows=None, rrows=None, lbase=0, rbase=0, kinds=J.KINDS, lcols=None, rcols=None, subkeys=None, case=None):
    """vl / vr: views whose projection columns lcols / rcols (default: all of lcomps / rcomps, in order) are the key components"""
    ql, qr = vl._query(), vr._query()
    lcols = list(range(len(lcomps))) if lcols is None else lcols
    rcols = list(range(len(rcomps))) if rcols is None else rcols
    before = (ql.count(), ql.indices().copy(), qr.count(), qr.indices().copy())
    want = JN.join_n_ref_all(lcomps, lrows, rcomps, rrows, lbase, rbase, kinds)
    for kind in kinds:
        wl, wr, winfo = want[kind]
        n, info = ql.join_count_n(qr, lcols, rcols, J.KIND_CODE[kind])
        assert n == len(wl) and info[:4] == winfo, (case, kind, n, len(wl), info, winfo)
        if subkeys is not None:
            assert info[5] == subkeys, (case, kind, info, subkeys)
        gl, gr = ql.join_fetch(n)
        assert gl.dtype == np.int64 and np.array_equal(gl, wl), (case, kind, gl[:8], wl[:8])
        assert np.array_equal(gr, wr), (case, kind, gr[:8], wr[:8])
    assert (ql.count(), qr.count()) == (before[0], before[2]) and np.array_equal(ql.indices(), before[1]) and np.array_equal(qr.indices(), before[3]), case


def check_sides(dfdb, ctx, lcomps, rcomps, **kw):
    tl, tr = table_of(dfdb, ctx, lcomps), table_of(dfdb, ctx, rcomps)
    check_views(keys_view(dfdb, tl, len(lcomps)), lcomps, keys_view(dfdb, tr, len(rcomps)), rcomps, **kw)
    tl.close()
    tr.close()


# ---------------------------------------------------------------- one key: the same answers as dfdb_query_join
def same_as_single(dfdb, ctx, left, right, case):
    tl, tr = table_of(dfdb, ctx, plain(left)), table_of(dfdb, ctx, plain(right))
    ql, qr = keys_view(dfdb, tl, 1)._query(), keys_view(dfdb, tr, 1)._query()
    for kind in J.KINDS:
        n1, info1 = ql.join_count(qr, 0, 0, J.KIND_CODE[kind])
        l1, r1 = ql.join_fetch(n1)
        n2, info2 = ql.join_count_n(qr, [0], [0], J.KIND_CODE[kind])
        l2, r2 = ql.join_fetch(n2)
        assert n1 == n2 and info1 == info2[:5], (case, kind, info1, info2)
        assert np.array_equal(l1, l2) and np.array_equal(r1, r2), (case, kind)
        assert info2[5] == (1 if len(left) and len(right) else 0), (case, info2)
    tl.close()
    tr.close()


def test_one_key_equals_dfdb_query_join(dfdb_mod, ctx):
    for dt in J.EDGE_DTYPES:
        left, right = J.edge_sides(dt, 300, 200)
        same_as_single(dfdb_mod, ctx, left, right, np.dtype(dt).name)
    right = J.unique_keys(1025)
    for nl in J.LEFT_COUNTS:
        same_as_single(dfdb_mod, ctx, J.probe_keys(nl, right), right, nl)


# ---------------------------------------------------------------- two fixed-width keys
def test_two_keys_left_row_counts(dfdb_mod, ctx):
    _, right = JN.pair_sides(0, 1025)
    tr = table_of(dfdb_mod, ctx, plain(*right))
    for nl in JN.LEFT_COUNTS_2:
        left, _ = JN.pair_sides(nl, 0)
        tl = table_of(dfdb_mod, ctx, plain(*left))
        check_views(keys_view(dfdb_mod, tl, 2), plain(*left), keys_view(dfdb_mod, tr, 2), plain(*right), subkeys=2 if nl else 0, case=nl)
        tl.close()
    tr.close()


def test_two_keys_right_row_counts(dfdb_mod, ctx):
    left, _ = JN.pair_sides(1025, 0)
    tl = table_of(dfdb_mod, ctx, plain(*left))
    for nr in JN.RIGHT_COUNTS_2:
        _, right = JN.pair_sides(0, nr)
        tr = table_of(dfdb_mod, ctx, plain(*right))
        check_views(keys_view(dfdb_mod, tl, 2), plain(*left), keys_view(dfdb_mod, tr, 2), plain(*right), subkeys=2 if nr else 0, case=nr)
        tr.close()
    tl.close()


def test_a_hot_major_key_and_a_unique_one(dfdb_mod, ctx):
    nr = 3000
    uniq = J.unique_keys(nr)
    probes = J.probe_keys(2100, uniq)
    hot_l, hot_r = np.full(2100, 5, np.int64), np.full(nr, 5, np.int64)
    # key 0 equal in every row: the second stage searches the whole right side
    check_sides(dfdb_mod, ctx, plain(hot_l, probes), plain(hot_r, uniq), case="hot major key")
    # the reverse: key 0 unique, every run has one row when the second stage begins
    check_sides(dfdb_mod, ctx, plain(probes, hot_l), plain(uniq, hot_r), case="unique major key")
    const_r = hot_r.copy(); const_r[::7] = 6
    check_sides(dfdb_mod, ctx, plain(probes, hot_l), plain(uniq, const_r), case="unique major key, minor differs")


def test_a_wave_mixes_empty_single_and_whole_runs(dfdb_mod, ctx):
    # right: 1900 rows of key 0 = 7 with key 1 unique, 100 rows whose key 0 is unique; left: within every 64 entries, key 0 absent (cnt = 0 after the first
    # stage), unique (cnt = 1), hot (cnt = 1900) and missing (cnt = 0 from the start, beside entries that start at cnt = nr)
    r0 = np.concatenate([np.full(1900, 7), np.arange(100, 200)]).astype(np.int64)
    r1 = np.concatenate([np.arange(1900), np.zeros(100)]).astype(np.int64)
    perm = np.random.default_rng(9).permutation(2000)
    r0, r1 = r0[perm], r1[perm]
    n = 1500
    rng = np.random.default_rng(10)
    l0 = np.array([7, 150, 999, 7], np.int64)[np.arange(n) % 4]
    l1 = np.where(l0 == 7, rng.integers(0, 2000, n), 0).astype(np.int64)
    lm = np.arange(n) % 4 == 3
    check_sides(dfdb_mod, ctx, [(l0, lm), (l1, None)], plain(r0, r1), case="mixed wave")


def test_the_greatest_tuple_ends_at_the_last_right_row(dfdb_mod, ctx):
    big = np.iinfo(np.int64).max
    for nr in (1, 64, 1025):
        r0 = np.full(nr, big, np.int64); r1 = np.full(nr, big, np.int64)
        r1[: nr // 2] = big - 1                                  # the run of (max, max) is the last of the order and ends at position nr
        l0 = np.full(6, big, np.int64); l1 = np.array([big, big - 1, big - 2, 0, -1, big], np.int64)
        l0[3] = big - 1
        check_sides(dfdb_mod, ctx, plain(l0, l1), plain(r0, r1), case=("int64", nr))
        ubig = np.iinfo(np.uint64).max
        check_sides(dfdb_mod, ctx, plain(np.array([True, True, False]), np.array([ubig, ubig - 1, ubig], np.uint64)),
                    plain(np.ones(nr, bool), np.full(nr, ubig, np.uint64)), case=("bool x uint64", nr))


def test_major_and_minor_keys_of_different_dtypes(dfdb_mod, ctx):
    for a, b in ((np.int8, np.float64), (np.bool_, np.uint64), (np.float32, np.int16), (np.uint8, np.float64)):
        la, ra = J.edge_sides(a, 700, 500)
        lb, rb = J.edge_sides(b, 700, 500)
        if np.dtype(a) == np.bool_:
            ra = la[:500].copy()                                 # (edge_sides leaves True out of a Bool right side: here both values are on both sides)
        check_sides(dfdb_mod, ctx, plain(la, lb), plain(ra, rb), case=(np.dtype(a).name, np.dtype(b).name))
        check_sides(dfdb_mod, ctx, plain(lb, la), plain(rb, ra), case=(np.dtype(b).name, np.dtype(a).name))


def test_three_keys_eight_keys_and_a_column_twice(dfdb_mod, ctx):
    rng = np.random.default_rng(33)
    nl, nr = 1100, 900
    dts = (np.int64, np.int8, np.float64, np.uint16, np.bool_, np.int32, np.uint64, np.float32)
    left = [rng.integers(0, 2, nl).astype(dt) for dt in dts]
    right = [rng.integers(0, 2, nr).astype(dt) for dt in dts]
    check_sides(dfdb_mod, ctx, plain(*left[:3]), plain(*right[:3]), subkeys=3, case="3 keys")
    check_sides(dfdb_mod, ctx, plain(*left), plain(*right), subkeys=8, case="8 keys")
    # a column twice: (k0, k1, k0) against (k0, k1, k0), and k0 against both of the other side's first two columns
    tl, tr = table_of(dfdb_mod, ctx, plain(*left[:2])), table_of(dfdb_mod, ctx, plain(*right[:2]))
    vl, vr = keys_view(dfdb_mod, tl, 2), keys_view(dfdb_mod, tr, 2)
    check_views(vl, plain(left[0], left[1], left[0]), vr, plain(right[0], right[1], right[0]), lcols=[0, 1, 0], rcols=[0, 1, 0], subkeys=3, case="a column twice")
    l8, r8 = left[0], right[0]
    check_views(vl, plain(l8, l8), vr, plain(r8, r8), lcols=[0, 0], rcols=[0, 0], kinds=("inner", "anti"), case="the same column as both keys")
    tl.close()
    tr.close()


# ---------------------------------------------------------------- String keys
def test_string_keys_alone_major_minor_and_two(dfdb_mod, ctx):
    for nl, nr in ((1023, 1025), (1024, 1024), (1025, 1023)):
        ls, rs = JN.string_sides(nl, nr)
        m = JN.chunks_of(rs)
        assert m == 32
        rng = np.random.default_rng([nl, nr])
        li, ri = rng.integers(0, 3, nl).astype(np.int64), rng.integers(0, 3, nr).astype(np.int64)
        ls2, rs2 = JN.string_sides(nl, nr, seed=8, drop=0)
        short_l, short_r = [s[:9] for s in ls2], [s[:9] for s in rs2]
        check_sides(dfdb_mod, ctx, [(ls, None)], [(rs, None)], subkeys=m + 1, case=("alone", nl, nr))
        check_sides(dfdb_mod, ctx, [(ls, None), (li, None)], [(rs, None), (ri, None)], subkeys=m + 2, kinds=("inner", "left"), case=("major", nl, nr))
        check_sides(dfdb_mod, ctx, [(li, None), (ls, None)], [(ri, None), (rs, None)], subkeys=m + 2, kinds=("semi", "anti", "inner"), case=("minor", nl, nr))
        check_sides(dfdb_mod, ctx, [(short_l, None), (ls, None)], [(short_r, None), (rs, None)], subkeys=JN.chunks_of(short_r) + 1 + m + 1, kinds=("inner", "anti"), case=("two", nl, nr))


def test_string_lengths_prefixes_and_nuls(dfdb_mod, ctx):
    pool = JN.string_pool()
    # every string of the pool on both sides, twice on the right; then each side without the other's longest strings
    check_sides(dfdb_mod, ctx, [(pool, None)], [(pool + pool[::-1], None)], subkeys=33, case="the pool against itself")
    short = [s for s in pool if len(s) <= 17]
    check_sides(dfdb_mod, ctx, [(pool, None)], [(short, None)], subkeys=JN.chunks_of(short) + 1, case="a right side of at most 17 bytes")
    assert JN.chunks_of(short) == 3
    for n in (8, 9, 16):                                          # m at the chunk boundary
        rs = [s for s in pool if len(s) <= n]
        check_sides(dfdb_mod, ctx, [(pool, None)], [(rs, None)], subkeys=(n + 7) // 8 + 1, kinds=("inner", "anti"), case=("longest", n))
    check_sides(dfdb_mod, ctx, [([b"", b"a", b""], None)], [([b"", b""], None)], subkeys=1, case="only empty strings on the right: m = 0")
    same = [b"constant key"] * 1500
    check_sides(dfdb_mod, ctx, [(same[:70] + [b"constant keY", b"constant ke", b"constant key\x00"], None)], [(same, None)], subkeys=3, case="an all-equal column")


def test_a_long_left_string_cannot_match_and_a_long_right_string_is_refused(dfdb_mod, ctx):
    from dfdb import _native as N
    base = bytes(range(1, 251)) * 5
    right = [base[:256], base[:255], b"x"]
    left = [base[:257], base[:1000], base[:256], b"x", base[:255]]
    check_sides(dfdb_mod, ctx, [(left, None)], [(right, None)], subkeys=33, case="left strings of 257 and 1000 bytes")
    tl, tr = table_of(dfdb_mod, ctx, [(left, None)]), table_of(dfdb_mod, ctx, [(right + [base[:257]], None), (np.arange(4, dtype=np.int64), None)])
    ql = keys_view(dfdb_mod, tl, 1)._query()
    n, _ = ql.join_count_n(keys_view(dfdb_mod, tr, 1, ("pred", "k1", "<", 3))._query(), [0], [0], dfdb_mod.JOIN_INNER)      # the long row is not selected
    assert n == 3
    rc, npairs, info = raw_join_n(ql, keys_view(dfdb_mod, tr, 1)._query(), [0], [0], 0)
    assert rc == N.ERR_UNSUPPORTED and "sorting by the String column k0 is not supported" in N.last_error() and "257 bytes" in N.last_error(), N.last_error()
    assert npairs == SENTINEL and np.all(info == SENTINEL)
    with pytest.raises(ValueError, match="has not been called"):                              # the failed call dropped the join that was pending
        ql.join_fetch(0)
    tl.close()
    tr.close()


def test_a_dictionary_column_on_either_side(dfdb_mod, ctx):
    ls, rs = JN.string_sides(1500, 700)
    li, ri = (np.arange(1500) % 2).astype(np.int64), (np.arange(700) % 2).astype(np.int64)
    for dl, dr in ((True, False), (False, True), (True, True)):
        tl, tr = table_of(dfdb_mod, ctx, [(ls, None), (li, None)]), table_of(dfdb_mod, ctx, [(rs, None), (ri, None)])
        if dl:
            assert tl.build_dictionary("k0") == len(set(ls))
        if dr:
            assert tr.build_dictionary("k0") == len(set(rs))
        check_views(keys_view(dfdb_mod, tl, 2), [(ls, None), (li, None)], keys_view(dfdb_mod, tr, 2), [(rs, None), (ri, None)], kinds=("inner", "anti"), case=(dl, dr))
        tl.close()
        tr.close()


# ---------------------------------------------------------------- missing components
def test_missing_components_match_nothing(dfdb_mod, ctx):
    (lx, lm), (rx, rm) = J.nullable_side(4097, 3, hi=12), J.nullable_side(3001, 4, hi=12)
    (ly, lm2), (ry, rm2) = J.nullable_side(4097, 6, hi=5), J.nullable_side(3001, 7, hi=5)
    for name, ml in (("key 0", (lm, None)), ("key 1", (None, lm2)), ("both", (lm, lm2))):
        for side in ("left", "right", "both"):
            lcomps = [(lx, ml[0] if side != "right" else None), (ly, ml[1] if side != "right" else None)]
            mr = {"key 0": (rm, None), "key 1": (None, rm2), "both": (rm, rm2)}[name]
            rcomps = [(rx, mr[0] if side != "left" else None), (ry, mr[1] if side != "left" else None)]
            check_sides(dfdb_mod, ctx, lcomps, rcomps, kinds=("inner", "left") if side == "both" else ("inner", "anti"), case=(name, side))
    whole_l = lm.copy(); whole_l[1024:2048] = True                                        # a whole missing tile
    whole_r = rm2.copy(); whole_r[1024:2048] = True
    check_sides(dfdb_mod, ctx, [(lx, whole_l), (ly, lm2)], [(rx, rm), (ry, whole_r)], case="a whole missing tile")
    check_sides(dfdb_mod, ctx, [(lx, np.ones(len(lx), bool)), (ly, None)], [(rx, rm), (ry, None)], kinds=("inner", "left"), case="every left row missing")
    check_sides(dfdb_mod, ctx, [(lx, lm), (ly, None)], [(rx, None), (ry, np.ones(len(ry), bool))], kinds=("inner", "anti"), subkeys=0, case="every right row missing")


def test_a_missing_string_beside_a_live_number(dfdb_mod, ctx):
    ls, rs = JN.string_sides(1300, 1100, seed=12)
    lmiss, rmiss = np.arange(1300) % 5 == 2, np.arange(1100) % 3 == 1
    li, ri = (np.arange(1300) % 3).astype(np.int64), (np.arange(1100) % 3).astype(np.int64)
    lcomps, rcomps = [(li, None), (JN.with_missing(ls, lmiss), None)], [(ri, None), (JN.with_missing(rs, rmiss), None)]
    want = JN.join_n_ref(lcomps, None, rcomps, None, "inner")[2]
    assert want[2] == int(lmiss.sum()) and want[3] == int(rmiss.sum())
    check_sides(dfdb_mod, ctx, lcomps, rcomps, case="String minor")
    check_sides(dfdb_mod, ctx, lcomps[::-1], rcomps[::-1], kinds=("inner", "left"), case="String major")
    (lx, lm), (rx, rm) = J.nullable_side(1300, 1, hi=3), J.nullable_side(1100, 2, hi=3)
    check_sides(dfdb_mod, ctx, [(lx, lm), (JN.with_missing(ls, lmiss), None)], [(rx, rm), (JN.with_missing(rs, rmiss), None)], kinds=("inner", "anti"), case="both nullable")
    check_sides(dfdb_mod, ctx, [([None] * 70, None)], [([None, b"a"] * 40, None)], kinds=("inner", "left"), case="every left String missing")


# ---------------------------------------------------------------- multiplicity
def test_multiplicity(dfdb_mod, ctx):
    for name, (left, right) in multiplicity_shapes().items():
        check_sides(dfdb_mod, ctx, plain(left, np.full(len(left), 4, np.int64)), plain(right, np.full(len(right), 4, np.int64)), case=name)
    # the first key's run of 5000 splits into runs of 1 to 70 by the second
    runs = np.repeat(np.arange(141), np.concatenate([np.arange(1, 71), np.arange(70, 0, -1), [30]]))[:5000].astype(np.int64)
    assert len(runs) == 5000
    r1 = runs[np.random.default_rng(2).permutation(5000)]
    l1 = np.arange(-2, 145, dtype=np.int64)
    check_sides(dfdb_mod, ctx, plain(np.full(len(l1), 3, np.int64), l1), plain(np.full(5000, 3, np.int64), r1), case="a run of 5000 splits")


# ---------------------------------------------------------------- selections and state
@pytest.fixture(scope="module")
def two_tables(dfdb_mod, ctx):
    n = 20_001
    rng = np.random.default_rng(n)
    k0 = rng.integers(0, 60, n).astype(np.int64)
    names = [f"brand{i}".encode() + b"x" * (i % 13) for i in range(40)]
    k1 = [names[i] for i in rng.integers(0, 40, n)]
    u = rng.integers(0, 100, n).astype(np.int64)
    tt = (np.arange(n) // 3000).astype(np.int64)
    big = table_of(dfdb_mod, ctx, [(k0, None), (k1, None)], extra=(("u", u), ("t", tt)))
    p0 = rng.integers(0, 60, 3000).astype(np.int64)
    p1 = [names[i] for i in rng.integers(0, 40, 3000)]
    small = table_of(dfdb_mod, ctx, [(p0, None), (p1, None)])
    return big, [(k0, None), (k1, None)], u, tt, small, [(p0, None), (p1, None)]


def test_selections_on_either_side_and_self_joins(dfdb_mod, ctx, two_tables):
    big, bcomps, u, tt, small, scomps = two_tables
    sels = K.selections(u, tt)
    for name in ("none", "range", "indices", "pred10", "nothing", "empty_tiles"):
        spec, rows = sels[name]
        kinds = J.KINDS if name in ("range", "nothing") else ("inner", "anti")
        check_views(keys_view(dfdb_mod, big, 2, spec), bcomps, keys_view(dfdb_mod, small, 2), scomps, lrows=rows, kinds=kinds, case=("left", name))
        check_views(keys_view(dfdb_mod, small, 2), scomps, keys_view(dfdb_mod, big, 2, spec), bcomps, rrows=rows, kinds=kinds, case=("right", name))
    spec, rows = sels["pred10"]
    spec2, rows2 = sels["empty_tiles"]
    check_views(keys_view(dfdb_mod, big, 2, spec), bcomps, keys_view(dfdb_mod, big, 2, spec2), bcomps, lrows=rows, rrows=rows2, kinds=("inner", "left"), case="self-join, two views")
    v = keys_view(dfdb_mod, big, 2, spec2)
    check_views(v, bcomps, v, bcomps, lrows=rows2, rrows=rows2, kinds=("inner", "semi"), case="self-join, one query")


def test_row_bases(dfdb_mod, ctx):
    l0, r0 = np.arange(2000, dtype=np.int64) % 700, np.arange(900, dtype=np.int64)
    l1, r1 = [b"s%d" % (i % 3) for i in range(2000)], [b"s%d" % (i % 2) for i in range(900)]
    tl, tr = table_of(dfdb_mod, ctx, [(l0, None), (l1, None)], extra=(("u", np.arange(2000, dtype=np.int64) % 3),)), table_of(dfdb_mod, ctx, [(r0, None), (r1, None)])
    tl.set_row_base(1 << 33)
    tr.set_row_base(65536 * 5)
    check_views(keys_view(dfdb_mod, tl, 2, ("pred", "u", "==", 1)), [(l0, None), (l1, None)], keys_view(dfdb_mod, tr, 2), [(r0, None), (r1, None)],
                lrows=np.arange(1, 2000, 3), lbase=1 << 33, rbase=65536 * 5)
    tl.close()
    tr.close()


@pytest.fixture(scope="module")
def frames(dfdb_mod, ctx):
    import pandas as pd
    rng = np.random.default_rng(78)
    nl, nr = 3000, 500
    brands = ["acme", "acm", "acme ", "żabka", "b", ""]
    left = pd.DataFrame({"k": rng.integers(0, 40, nl).astype(np.int64), "brand": [brands[i] for i in rng.integers(0, 6, nl)], "a": rng.standard_normal(nl),
                         "s": [f"row{i % 97}" + "x" * (i % 11) for i in range(nl)]})
    right = pd.DataFrame({"k": rng.integers(0, 40, nr).astype(np.int64), "brand": [brands[i] for i in rng.integers(0, 5, nr)], "b": rng.integers(-5, 5, nr).astype(np.int32),
                          "name": [f"r{i}" for i in range(nr)]})
    tl = dfdb_mod.DFTable.from_columns({c: (left[c].tolist() if isinstance(left[c].iloc[0], str) else left[c].to_numpy()) for c in left}, ctx=ctx)
    tr = dfdb_mod.DFTable.from_columns({c: (right[c].tolist() if isinstance(right[c].iloc[0], str) else right[c].to_numpy()) for c in right}, ctx=ctx)
    return tl, left, tr, right


def frame_comps(df, cols):
    return [((df[c].tolist() if isinstance(df[c].iloc[0], str) else df[c].to_numpy()), None) for c in cols]


def test_device_lists_feed_the_gathers(dfdb_mod, ctx, frames):
    import torch
    from dfdb.api import _flat_to_strings
    tl, left, tr, right = frames
    v, w = tl[dfdb_mod.ALL, dfdb_mod.ALL], tr[("b", lambda b: b < 3), dfdb_mod.ALL]
    ql = v._query()
    n, info = ql.join_count_n(w._query(), [0, 1], [0, 1], dfdb_mod.JOIN_INNER)
    wl, wr, winfo = JN.join_n_ref(frame_comps(left, ["k", "brand"]), None, frame_comps(right, ["k", "brand"]), np.flatnonzero((right["b"] < 3).to_numpy()), "inner")
    assert n == len(wl) and n > 0 and info[:4] == winfo
    w._q = None                                                                           # the right query is freed between call 1 and the fetch
    buf = torch.full((2, n + 2), SENTINEL, dtype=torch.int64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    for _ in range(2):                                                                    # and the fetch is repeated
        ql.join_fetch(n, (buf[0].data_ptr() + 8, buf[1].data_ptr() + 8))
        ctx.synchronize()
        h = buf.cpu().numpy()
        assert np.all(h[:, 0] == SENTINEL) and np.all(h[:, -1] == SENTINEL) and np.array_equal(h[0, 1:-1], wl) and np.array_equal(h[1, 1:-1], wr)
    lcols = ql.gather_rows_any(dev_ptr=buf[0].data_ptr() + 8, n=n)                        # the rows never leave the device; `s` is a String payload
    assert np.array_equal(lcols[0], left["k"].to_numpy()[wl - 1]) and _flat_to_strings(*lcols[3]) == left["s"].to_numpy()[wl - 1].tolist()
    rcols = tr[dfdb_mod.ALL, dfdb_mod.ALL]._query().gather_rows_any(dev_ptr=buf[1].data_ptr() + 8, n=n)
    assert np.array_equal(rcols[2], right["b"].to_numpy()[wr - 1]) and _flat_to_strings(*rcols[3]) == right["name"].to_numpy()[wr - 1].tolist()
    lt, rt, info2 = ql.join(tr[dfdb_mod.ALL, dfdb_mod.ALL]._query(), [1, 0], [1, 0], dfdb_mod.JOIN_SEMI, device=True)
    ctx.synchronize()
    ws = JN.join_n_ref(frame_comps(left, ["brand", "k"]), None, frame_comps(right, ["brand", "k"]), None, "semi")
    assert np.array_equal(lt.cpu().numpy(), ws[0]) and np.array_equal(rt.cpu().numpy(), ws[1]) and info2[:4] == ws[2]


def test_frames_with_a_list_on_against_pandas_merge(dfdb_mod, ctx, frames):
    tl, left, tr, right = frames
    v, w = tl[("a", lambda a: a < 0.5), dfdb_mod.ALL], tr[dfdb_mod.ALL, dfdb_mod.ALL]
    lsel = left[left["a"] < 0.5]
    frame_equal(dfdb_mod.innerjoin(v, w, ["k", "brand"]), lsel.merge(right, on=["k", "brand"], how="inner", sort=False))
    frame_equal(dfdb_mod.innerjoin(v, tr[dfdb_mod.ALL, ["brand", "b", "name"]], "brand"), lsel.merge(right[["brand", "b", "name"]], on="brand", how="inner", sort=False))   # a String `on`
    rkeys = set(zip(right["k"].tolist(), right["brand"].tolist()))
    has = np.array([k in rkeys for k in zip(lsel["k"].tolist(), lsel["brand"].tolist())])
    frame_equal(dfdb_mod.semijoin(v, w, ["k", "brand"]), lsel[has])
    frame_equal(dfdb_mod.antijoin(v, w, [("k", "k"), "brand"]), lsel[~has])
    w2 = tr[dfdb_mod.ALL, ["name", "brand", "k"]]                                          # pairs of names; the right key columns are dropped where they stand
    frame_equal(dfdb_mod.innerjoin(v, w2, [("brand", "brand"), ("k", "k")]),
                lsel.merge(right[["name", "brand", "k"]], on=["brand", "k"], how="inner", sort=False)[["k", "brand", "a", "s", "name"]])
    gl, gr, info = dfdb_mod.join_rows(v, w, ["brand", "k"], kind="left")
    wl, wr, winfo = JN.join_n_ref(frame_comps(left, ["brand", "k"]), np.flatnonzero((left["a"] < 0.5).to_numpy()), frame_comps(right, ["brand", "k"]), None, "left")
    assert np.array_equal(gl, wl) and np.array_equal(gr, wr) and info[:4] == winfo and len(info) == 6
    gl1, gr1, info1 = dfdb_mod.join_rows(v, w, "k", kind="inner")                          # a single fixed-width `on` keeps calling dfdb_query_join
    assert len(info1) == 5
    with pytest.raises(ValueError, match="Duplicate variable names: a"):
        dfdb_mod.innerjoin(tl[dfdb_mod.ALL, ["k", "brand", "a"]], tl[dfdb_mod.ALL, ["k", "brand", "a"]], ["k", "brand"])
    with pytest.raises(KeyError):
        dfdb_mod.join_rows(v, w, ["k", "nope"])
    with pytest.raises(ValueError, match="on ="):
        dfdb_mod.join_rows(v, w, [])


def test_matchmissing_names_the_side(dfdb_mod, ctx):
    ls, rs = JN.string_sides(500, 300, seed=4)
    lmiss, rmiss = np.arange(500) % 5 == 1, np.arange(300) % 5 == 2
    li, ri = (np.arange(500) % 2).astype(np.int64), (np.arange(300) % 2).astype(np.int64)
    tl = table_of(dfdb_mod, ctx, [(li, None), (JN.with_missing(ls, lmiss), None)])
    tr = table_of(dfdb_mod, ctx, [(ri, None), (JN.with_missing(rs, rmiss), None)])
    tp = table_of(dfdb_mod, ctx, [(ri, None), (rs, None)])
    for a, b, side in ((tl, tp, "left"), (tp, tr, "right"), (tl, tr, "left")):
        with pytest.raises(ValueError, match="missing values in the key columns of the %s side" % side):
            dfdb_mod.join_rows(a, b, ["k0", "k1"])
    gl, gr, info = dfdb_mod.join_rows(tl, tr, ["k0", "k1"], matchmissing="notequal")
    wl, wr, winfo = JN.join_n_ref([(li, None), (JN.with_missing(ls, lmiss), None)], None, [(ri, None), (JN.with_missing(rs, rmiss), None)], None, "inner")
    assert np.array_equal(gl, wl) and np.array_equal(gr, wr) and info[:4] == winfo and winfo[2] == 100 and winfo[3] == 60
    for t in (tl, tr, tp):
        t.close()


def raw_join_n(ql, qr, lcols, rcols, kind, nkeys=None):
    """the raw call with sentinel-filled outputs: (status, npairs, info); lcols / rcols None: a null list"""
    from dfdb import _native as N
    n = C.c_int64(SENTINEL)
    info = np.full(6, SENTINEL, np.int64)
    lc = None if lcols is None else np.ascontiguousarray(lcols, np.int32)
    rc = None if rcols is None else np.ascontiguousarray(rcols, np.int32)
    nk = nkeys if nkeys is not None else len(lc)
    rc_ = N.load().dfdb_query_join_n(ql._h, None if lc is None else lc.ctypes.data, qr._h, None if rc is None else rc.ctypes.data, nk, kind, C.byref(n), info.ctypes.data)
    return rc_, n.value, info


def test_pending_state(dfdb_mod, ctx, tmp_path):
    from dfdb import _native as N
    ls, rs = JN.string_sides(2000, 900, seed=21)
    li, ri = (np.arange(2000) % 4).astype(np.int64), (np.arange(900) % 4).astype(np.int64)
    lcomps, rcomps = [(li, None), (ls, None)], [(ri, None), (rs, None)]
    tl, tr = table_of(dfdb_mod, ctx, lcomps), table_of(dfdb_mod, ctx, rcomps)
    ql, qr = keys_view(dfdb_mod, tl, 2)._query(), keys_view(dfdb_mod, tr, 2)._query()
    L = N.load()
    lr, rr = np.full(200_000, SENTINEL, np.int64), np.full(200_000, SENTINEL, np.int64)

    def nothing_pending():
        assert L.dfdb_query_join_fetch(ql._h, lr.ctypes.data, rr.ctypes.data, len(lr), N.MEM_HOST) == N.ERR_ARGUMENT and "has not been called" in N.last_error()
        assert np.all(lr == SENTINEL) and np.all(rr == SENTINEL)

    nothing_pending()
    want = JN.join_n_ref_all(lcomps, None, rcomps, None)
    n, _ = ql.join_count_n(qr, [0, 1], [0, 1], dfdb_mod.JOIN_LEFT)
    for _ in range(2):                                                                     # a fetch may be repeated
        gl, gr = ql.join_fetch(n)
        assert np.array_equal(gl, want["left"][0]) and np.array_equal(gr, want["left"][1])
    assert L.dfdb_query_join_fetch(ql._h, lr.ctypes.data, rr.ctypes.data, n - 1, N.MEM_HOST) == N.ERR_BOUNDS and np.all(lr == SENTINEL)
    n2, _ = ql.join_count_n(qr, [0, 1], [0, 1], dfdb_mod.JOIN_SEMI)                        # the next successful call replaces it
    gl, gr = ql.join_fetch(n2)
    assert np.array_equal(gl, want["semi"][0]) and np.array_equal(gr, want["semi"][1])
    n3, _ = ql.join_count(qr, 0, 0, dfdb_mod.JOIN_SEMI)                                    # and so does dfdb_query_join, whose lists the same fetch writes
    assert n3 == 2000
    assert raw_join_n(ql, qr, [0, 1], [1, 0], 0)[0] == N.ERR_UNSUPPORTED                   # a failed call drops it
    nothing_pending()
    ql.join_count_n(qr, [0, 1], [0, 1], dfdb_mod.JOIN_INNER)
    ql.reset()                                                                             # dfdb_query_reset drops it
    nothing_pending()
    tl.save(str(tmp_path / "left"))                                                        # dfdb_table_unload (a table with backing files) drops it
    tf = dfdb_mod.open_table(str(tmp_path / "left"), ctx=ctx)
    ql = keys_view(dfdb_mod, tf, 2)._query()
    n4, _ = ql.join_count_n(qr, [0, 1], [0, 1], dfdb_mod.JOIN_LEFT)
    assert n4 == n and np.array_equal(ql.join_fetch(n4)[1], want["left"][1])
    N.check(L.dfdb_table_unload(tf._h, None, 0))
    nothing_pending()
    tf.close()
    tr.close()
    tl.close()


def test_refusals_name_the_form_and_touch_nothing(dfdb_mod, ctx, tmp_path):
    from dfdb import _native as N
    x = (np.arange(5000, dtype=np.int64) * 7919) % 1009
    t = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    add_raw(dfdb_mod, t, "x", x)
    t.add_column("s", ["a", "b", "c", "d"] * 1250)
    add_raw(dfdb_mod, t, "f", x.astype(np.float64))
    add_raw(dfdb_mod, t, "i", x.astype(np.int32))
    both = t[dfdb_mod.ALL, ["x", "s", "f", "i"]]
    good = both._query()

    def refused(ql, qr, lcols, rcols, kind, status, pattern, nkeys=None):
        rc, n, info = raw_join_n(ql, qr, lcols, rcols, kind, nkeys)
        assert rc == status and pattern in N.last_error() and n == SENTINEL and np.all(info == SENTINEL), (pattern, rc, N.last_error())

    refused(good, good, [0, 1], [0, 2], 0, N.ERR_UNSUPPORTED, "key 1: String and Float64")
    refused(good, good, [0, 2], [0, 1], 0, N.ERR_UNSUPPORTED, "key 1: Float64 and String")
    refused(good, good, [3, 0], [0, 0], 0, N.ERR_UNSUPPORTED, "key 0: Int32 and Int64")
    refused(good, good, [0, 0, 2], [0, 0, 3], 0, N.ERR_UNSUPPORTED, "key 2: Float64 and Int32")
    computed = t[dfdb_mod.ALL, "x"] + 1
    refused(computed.view._query(), good, [0], [0], 0, N.ERR_UNSUPPORTED, "joining on a computed column")
    refused(good, computed.view._query(), [0], [0], 0, N.ERR_UNSUPPORTED, "joining on a computed column")
    for kind in (-1, 4, 99):
        refused(good, good, [0, 1], [0, 1], kind, N.ERR_ARGUMENT, "join kind")
    for nkeys in (0, -1, 9):
        refused(good, good, [0] * 9, [0] * 9, 0, N.ERR_ARGUMENT, "join keys (1 to 8)", nkeys=nkeys)
    refused(good, good, None, [0], 0, N.ERR_ARGUMENT, "no left key columns", nkeys=1)
    refused(good, good, [0], None, 0, N.ERR_ARGUMENT, "no right key columns", nkeys=1)
    for lc, rc_col in (([0, 4], [0, 0]), ([0, 0], [0, -1])):
        rc, n, info = raw_join_n(good, good, lc, rc_col, 0)
        assert rc == N.ERR_BOUNDS and n == SENTINEL and np.all(info == SENTINEL)
    other = dfdb_mod.Context(0)                                                            # queries of two contexts
    t2 = dfdb_mod.DFTable.new(block_size=65536, ctx=other)
    add_raw(dfdb_mod, t2, "x", x)
    refused(good, t2[dfdb_mod.ALL, ["x"]]._query(), [0], [0], 0, N.ERR_ARGUMENT, "different contexts")
    n, info = good.join_count_n(good, [1, 0], [1, 0], dfdb_mod.JOIN_INNER)                 # the same views are fine when the types agree
    assert info[:4] == (5000, 5000, 0, 0) and info[5] == 3
    # a view that is out of core: the table's files, opened without loading
    t.save(str(tmp_path / "tb"))
    tf = dfdb_mod.open_table(str(tmp_path / "tb"), ctx=ctx, load=False)
    for a, b in ((tf[dfdb_mod.ALL, ["x", "s"]], t[dfdb_mod.ALL, ["x", "s"]]), (t[dfdb_mod.ALL, ["x", "s"]], tf[dfdb_mod.ALL, ["x", "s"]])):
        refused(a._query(), b._query(), [0, 1], [0, 1], 0, N.ERR_UNSUPPORTED, "out of core")
    tf.close()
    t.compress_column("x", 2)                                                              # what keep_compressed = 2 leaves: the LZ4 blocks alone
    v = t[dfdb_mod.ALL, ["s", "x"]]
    refused(v._query(), v._query(), [0, 1], [0, 1], 0, N.ERR_UNSUPPORTED, "compressed-only")
    t2.close()
    other.close()
    t.close()


def test_a_table_of_2_to_31_rows_is_refused_on_either_side(dfdb_mod, ctx):
    """rows travel in 32 bits with the top bit spare: a table of 2^31 rows is refused by name on the left, on the right and on both, before anything is
    launched (no selection is executed), with nothing left pending.  The column is generated on the device (17 GB, no host copy)"""
    from dfdb import _native as N
    big = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    big.add_generated("x", dfdb_mod.GEN_I64_IOTA, 0, 1 << 31)
    small = dfdb_mod.DFTable.new(block_size=65536, ctx=ctx)
    add_raw(dfdb_mod, small, "x", np.arange(100, dtype=np.int64))
    qb, qs = big[dfdb_mod.ALL, ["x"]]._query(), small[dfdb_mod.ALL, ["x"]]._query()
    n, _ = qs.join_count_n(qs, [0, 0], [0, 0], dfdb_mod.JOIN_INNER)                        # a join is pending in the small query: the refused calls drop it
    assert n == 100
    lr = np.full(128, SENTINEL, np.int64)
    for ql, qr, side in ((qb, qs, "left"), (qs, qb, "right"), (qb, qb, "left")):
        rc, n, info = raw_join_n(ql, qr, [0, 0], [0, 0], 0)
        assert rc == N.ERR_UNSUPPORTED and "joining a table of 2^31 rows or more (the %s side)" % side in N.last_error(), (side, rc, N.last_error())
        assert n == SENTINEL and np.all(info == SENTINEL), side
        assert N.load().dfdb_query_join_fetch(ql._h, lr.ctypes.data, None, 128, N.MEM_HOST) == N.ERR_ARGUMENT and "has not been called" in N.last_error(), side
        assert np.all(lr == SENTINEL), side
    del qb
    big.close()
    small.close()


def test_the_2_to_32_boundary(dfdb_mod, ctx):
    """1024 consecutive left rows may have 2^32 - 1 pairs between them and no more: call 1 only, nothing is fetched"""
    tl = table_of(dfdb_mod, ctx, plain(np.full(1024, 9, np.int64), np.full(1024, 2, np.int8)))
    ql = keys_view(dfdb_mod, tl, 2)._query()
    for nr, ok in ((4_194_303, True), (4_194_304, False)):
        tr = table_of(dfdb_mod, ctx, plain(np.full(nr, 9, np.int64), np.full(nr, 2, np.int8)))
        qr = keys_view(dfdb_mod, tr, 2)._query()
        if ok:
            n, info = ql.join_count_n(qr, [0, 1], [0, 1], dfdb_mod.JOIN_INNER)
            assert n == (1 << 32) - 1024 and info == (1024, nr, 0, 0, 0, 2)               # an all-equal right side sorts in 0 passes
        else:
            with pytest.raises(NotImplementedError, match=r"more than 2\^32 - 1 pairs from 1024 consecutive left rows"):
                ql.join_count_n(qr, [0, 1], [0, 1], dfdb_mod.JOIN_INNER)
            with pytest.raises(ValueError, match="has not been called"):                   # the refused call left nothing pending
                ql.join_fetch(0)
            assert ql.join_count_n(qr, [0, 1], [0, 1], dfdb_mod.JOIN_SEMI)[0] == 1024     # the other kinds of the same sides fit
        tr.close()
    tl.close()


def test_launch_counts_from_the_profile(dfdb_mod, ctx):
    names = ("join_refine", "join_probe", "join_expand", "join_live", "sort_rows", "sort_rekey", "sort_strkey", "sort_strkey_len")
    left = [b"abcdefghij", b"abcdefghi", b"k"] * 700                                        # m = 2 on the right
    right = [b"abcdefghij", b"abcdefghiJ", b"q"] * 300
    li, ri = (np.arange(2100) % 2).astype(np.int64), (np.arange(900) % 2).astype(np.int64)
    tl, tr = table_of(dfdb_mod, ctx, [(li, None), (left, None)]), table_of(dfdb_mod, ctx, [(ri, None), (right, None)])
    ql, qr = keys_view(dfdb_mod, tl, 2)._query(), keys_view(dfdb_mod, tr, 2)._query()
    assert (ql.count(), qr.count()) == (2100, 900)
    (n, info), c = counted(ctx, names, lambda: ql.join_count_n(qr, [0, 1], [0, 1], dfdb_mod.JOIN_INNER))
    assert n == 700 * 150 and info[:4] == (2100, 900, 0, 0) and info[5] == 4
    # one refine launch per sub-key (Int64, chunk 0, chunk 1, length); the right sub-keys by the sort's own kernels: the sort's 1 + 3 launches and the stages' 1 + 3;
    # no key is nullable: one live walk (the left side's first ranges)
    assert c == {"join_refine": 4, "join_probe": 0, "join_expand": 0, "join_live": 1, "sort_rows": 2, "sort_rekey": 2, "sort_strkey": 4, "sort_strkey_len": 2}, c
    (gl, gr), c = counted(ctx, names, lambda: ql.join_fetch(n))
    assert c["join_expand"] == 1 and c["join_refine"] == 0 and len(gl) == n
    # no right row: no stage and no sub-key launch; the kinds' totals still come out
    empty = keys_view(dfdb_mod, tr, 2, ("pred", "k0", "<", 0))._query()
    assert empty.count() == 0
    (got, c) = counted(ctx, names, lambda: [ql.join_count_n(empty, [0, 1], [0, 1], k)[0] for k in range(4)])
    assert got == [0, 2100, 0, 2100] and c["join_refine"] == 0 and c["sort_rekey"] == 0 and c["sort_strkey"] == 0, (got, c)
    gl, gr = ql.join_fetch(2100)
    assert np.array_equal(gl, np.arange(1, 2101)) and not gr.any()
    # every right row missing in one component: the same
    tm = table_of(dfdb_mod, ctx, [(ri, np.ones(900, bool)), (right, None)])
    (n, info), c = counted(ctx, names, lambda: ql.join_count_n(keys_view(dfdb_mod, tm, 2)._query(), [0, 1], [0, 1], dfdb_mod.JOIN_LEFT))
    assert n == 2100 and info == (2100, 900, 0, 900, info[4], 0) and c["join_refine"] == 0 and c["join_live"] == 3, (info, c)
    for t in (tl, tr, tm):
        t.close()
