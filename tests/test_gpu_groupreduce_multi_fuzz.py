"""groupreduce by a tuple of key columns (dfdb_query_groupreduce_n) over the random selection queues of the differential fuzz, and its dispatch edges on purpose.

The fixed shapes of test_gpu_groupreduce_multi.py always select with one predicate on a Float64 column; here the queue in front is random (ranges, index
lists, predicates: partial bitmap words, restore_group_selection behind a range stage), the table is flat, dictionary-coded or compressed-only, and unique's
knobs force table growth, migration, the dense span form and one-tile chunks under group_rank_key.  The yardstick is `expect` of test_gpu_groupreduce_multi.py
(numpy, groups by first appearance of the isequal image of the tuple) with Float sums from math.fsum per group: exact, rounded once.  Counts, keys, integer
results (wrapping) and min / max are compared exactly; Float sums within count * eps * sum|x| per group (divided by count for a mean).

Float64 sums of a group start from +0.0, as the reference's `Sum()` reducer does: a group of -0.0 alone sums to +0.0."""
import os
import types

import numpy as np
import pytest

from helpers import _oracle_view, apply_stages_both
from test_gpu_fuzz import BLOCK, SCALE, SEED0, Gen, GenNoMissing, filed, full_columns, pair, pair_columns_host  # noqa: F401  (pair, filed: fixtures)
from test_gpu_groupreduce_multi import check_frame, expect, run_case

gpu = pytest.mark.gpu

KEY_COLS = ["a", "i8", "s", "m", "c", "i32", "u64", "x", "flag", "sm", "u16"]
VAL_COLS = ["a", "b", "i32", "u16", "x", "f", "i8", "u64"]
STATS = ["count", "sum", "min", "max", "mean"]
SEED_BASE, REDRAWS = 130_000, 3
NSEEDS, NSTREAMED = 100 * SCALE, 40 * SCALE
KNOB_DEFAULTS = {"unique_dense": 1, "unique_cap0_log2": 21, "unique_chunk_tiles": 0, "unique_dense_range": 1 << 40}
KNOB_SETS = [{}, {"unique_dense": 0}, {"unique_dense": 0, "unique_cap0_log2": 10, "unique_chunk_tiles": 1}, {"unique_dense_range": 100, "unique_chunk_tiles": 1}]


def selection_mask(ov, n):
    sel = np.zeros(n, bool)
    sel[ov.select_indices() - 1] = True
    return sel


def draw_once(gen, key_cols):
    """stages, 1-4 key columns without repetition, 0-6 reducers (the same column may come back under another statistic)"""
    stages = gen.stages()
    by = [key_cols[int(i)] for i in gen.rng.permutation(len(key_cols))[:int(gen.rng.integers(1, 5))]]
    reds = {}
    for j in range(int(gen.rng.integers(0, 7))):
        stat, col = gen.pick(STATS), gen.pick(VAL_COLS)
        reds["r%d" % j] = (None if stat == "count" else col, stat)
    return stages, by, reds


def draw_case(ir, seed, host, gen_cls=Gen, key_cols=KEY_COLS, base=SEED_BASE):
    """Gen.stages() ends in an integer stage, a short index list or an empty selection for four queues in ten (43 of the first 100), which would leave
    groupreduce one group or none to number.  The case of a seed is therefore the first of REDRAWS draws for which the ORACLE (host.o: the reference alone, the
    engine is not asked) builds the queue and selects at least two distinct key tuples, else the last draw: empty selections, single groups and refused queues
    stay in the mix, under the caps that test_the_seeds_reach_groups_host_side asserts."""
    for attempt in range(REDRAWS):
        case = draw_once(gen_cls(ir, base + REDRAWS * seed + attempt, risky=False), key_cols)
        try:
            ov = _oracle_view(host, case[0], None)
        except Exception:      # noqa: BLE001 — refused when the queue is built
            continue
        cols = full_columns(host)
        if len(expect([cols[b] for b in case[1]], selection_mask(ov, host.nrows), {})[1]) >= 2:
            break
    return case


def host_reducers(cols, reds):
    return {nm: (None if c is None else np.ma.getdata(cols[c]), stat) for nm, (c, stat) in reds.items()}


def same_frames(a, b, reds, tag):
    """keys, counts and every column that is not a Float sum: equal bit for bit (Float sums are atomic adds in no fixed order: each frame is held to the bound)"""
    assert list(a.columns) == list(b.columns) and len(a) == len(b), tag
    loose = {nm for nm, (c, stat) in reds.items() if stat in ("sum", "mean") and c in ("x", "f")}
    for c in a.columns:
        if c in loose:
            continue
        x, y = a[c].to_numpy(), b[c].to_numpy()
        if x.dtype.kind == "f":                                # (NaN is NaN; every other value bit for bit, the sign of a zero included)
            assert np.array_equal(np.isnan(x), np.isnan(y)), (tag, c)
            assert np.where(np.isnan(x), 0.0, x).tobytes() == np.where(np.isnan(y), 0.0, y).tobytes(), (tag, c)
        else:
            assert x.tolist() == y.tolist(), (tag, c)


# ---------------------------------------------------------------- the cap: the seeds must not be mostly empty selections, single groups or refused queues
def test_the_seeds_reach_groups_host_side(oracle):
    """Walks every seed with the oracle alone: at most 15 % of them end with an empty selection or a single group, at most 5 % are refused when the queue is
    built (what the GPU test may skip, and only when the engine refuses too).  With SEED_BASE = 130000, REDRAWS = 3 and the default 100 seeds: 6 seeds with
    fewer than two groups (3 of them empty selections), none refused; a single draw per seed gave 43."""
    from dfdb import ir
    cols = pair_columns_host()
    ot = oracle.Table(block_size=BLOCK)
    for k, v in cols.items():
        if isinstance(v, np.ma.MaskedArray):
            ot.add_column(k, np.ascontiguousarray(v.filled(0)), missing=np.ma.getmaskarray(v))
        else:
            ot.add_column(k, v)
    host = types.SimpleNamespace(o=ot, O=oracle, names=list(cols), nrows=len(cols["a"]))
    full = full_columns(host)
    refused = few = empty = 0
    for seed in range(SEED0, SEED0 + NSEEDS):
        stages, by, reds = draw_case(ir, seed, host)
        try:
            ov = _oracle_view(host, stages, None)
        except Exception:      # noqa: BLE001 — a queue refused at build time
            refused += 1
            continue
        sel = selection_mask(ov, host.nrows)
        ng = len(expect([full[b] for b in by], sel, {})[1])
        few += ng < 2
        empty += ng == 0
    print("seeds %d: refused %d, fewer than two groups %d (empty %d)" % (NSEEDS, refused, few, empty))
    assert few <= 0.15 * NSEEDS, (few, NSEEDS)
    assert refused <= 0.05 * NSEEDS, (refused, NSEEDS)


# ---------------------------------------------------------------- random queues, resident
@gpu
@pytest.mark.parametrize("seed", range(SEED0, SEED0 + NSEEDS))
def test_random_tuple_groupreduce(pair, dfdb_mod, seed):
    from dfdb import api, ir
    stages, by, reds = draw_case(ir, seed, pair)
    ctx0 = dfdb_mod.default_context(0)
    for k, v in {**KNOB_DEFAULTS, **KNOB_SETS[seed % 4]}.items():
        ctx0.set_option(k, int(v))
    try:
        ov, dv = apply_stages_both(pair, stages)      # skips only when oracle AND engine refuse the queue with the same exception class; a one-sided refusal fails
        cols = full_columns(pair)
        sel = selection_mask(ov, pair.nrows)
        keys, hreds, tag = [cols[b] for b in by], host_reducers(cols, reds), (seed, stages, by, reds)
        before_n, before_idx = dfdb_mod.nrow(dv), dv._query().indices().copy()
        assert before_n == int(sel.sum()), tag
        df = dfdb_mod.groupreduce(dv, tuple(by), **reds)
        check_frame(df, by, keys, sel, hreds, tag, exact_float_sums=True)
        # the view's own query still answers for the whole selection
        assert dfdb_mod.nrow(dv) == before_n and np.array_equal(dv._query().indices(), before_idx), tag
        # two calls on ONE query handle: the selection is restored after each fetch, the second frame equals the first
        names = list(by) + [c for c, st in reds.values() if st != "count" and c not in by]
        names = list(dict.fromkeys(names))
        q = api._Query(api.DFView(dv.table, api.Projection({nm: dv.projection.cols[nm] for nm in names}), dv.selection))
        vidx = [names.index(c) if st != "count" else -1 for c, st in reds.values()]
        stats = [st for _, st in reds.values()]
        r1 = api._groupreduce_n_raw(q, len(by), vidx, stats)
        assert q.count() == before_n and np.array_equal(q.indices(), before_idx), tag
        r2 = api._groupreduce_n_raw(q, len(by), vidx, stats)
        assert q.count() == before_n and np.array_equal(q.indices(), before_idx), tag
        assert np.array_equal(r1[1], r2[1]) and np.array_equal(r1[1], df["count"].to_numpy()), tag
        for i, (c, st) in enumerate(reds.values()):
            if st in ("sum", "mean") and c in ("x", "f"):
                continue                                       # (atomic Float adds: each call is held to the bound through dfdb.groupreduce above and below)
            assert np.array_equal(r1[2][i], r2[2][i]) and r1[3][i].tobytes() == r2[3][i].tobytes(), (tag, i)
        df2 = dfdb_mod.groupreduce(dv, tuple(by), **reds)
        check_frame(df2, by, keys, sel, hreds, tag, exact_float_sums=True)
        same_frames(df, df2, reds, tag)
    finally:
        for k, v in KNOB_DEFAULTS.items():
            ctx0.set_option(k, v)


# ---------------------------------------------------------------- random queues, block-streamed from the files
@gpu
@pytest.mark.parametrize("seed", range(SEED0, SEED0 + NSTREAMED))
def test_random_tuple_groupreduce_streamed(filed, dfdb_mod, seed):
    """the table that is not resident (ooc_chunk_blocks 1-5: the chunks' groups merged in chunk order) against the resident call and against the reference"""
    from dfdb import ir
    pair_f, lazy, _ = filed
    keyc = [c for c in KEY_COLS if c not in ("m", "sm")]                 # (`filed` has no nullable column)
    stages, by, reds = draw_case(ir, seed, pair_f, GenNoMissing, keyc, SEED_BASE + 500_000)
    ov, dv = apply_stages_both(pair_f, stages)      # skips only when oracle AND engine refuse the queue with the same exception class; a one-sided refusal fails
    cols = full_columns(pair_f)
    sel = selection_mask(ov, pair_f.nrows)
    keys, hreds, tag = [cols[b] for b in by], host_reducers(cols, reds), (seed, stages, by, reds)
    res = dfdb_mod.groupreduce(dv, tuple(by), **reds)
    check_frame(res, by, keys, sel, hreds, tag, exact_float_sums=True)
    lazy.ctx.set_option("ooc_chunk_blocks", 1 + seed % 5)
    try:
        ooc = dfdb_mod.groupreduce(dfdb_mod.DFView(lazy, None, dv.selection), tuple(by), **reds)
        assert not lazy.resident(0), tag
    finally:
        lazy.ctx.set_option("ooc_chunk_blocks", 512)
    check_frame(ooc, by, keys, sel, hreds, tag, exact_float_sums=True)
    same_frames(ooc, res, reds, tag)


# ---------------------------------------------------------------- the rank kernels' forms on purpose
def _span_key(rng, n, span, nullable):
    """an Int64 key whose values cover [lo, lo + span - 1] exactly, both ends on many rows (a filtered view keeps them)"""
    lo = -span // 2
    k = rng.integers(lo, lo + span, n).astype(np.int64)
    ends = rng.permutation(n)[:128]
    k[ends[:64]], k[ends[64:]] = lo, lo + span - 1
    if not nullable:
        return k
    mask = rng.random(n) < 0.03
    mask[ends] = False
    mask[:64] = False                                      # (missing is not the first group: its rank is not 0)
    return np.ma.masked_array(k, mask=mask)


@gpu
@pytest.mark.parametrize("place", ["first", "second"])
@pytest.mark.parametrize("nullable", [False, True], ids=["plain", "nullable"])
@pytest.mark.parametrize("span", [16000, 16001])
def test_rank_table_in_lds_at_its_limit(dfdb_mod, ctx, span, nullable, place):
    """a dense key of exactly kRankLdsRange = 16000 values (k_group_rank<3>: the table in LDS, the missing key's rank in the slot behind it) and of one more
    (k_group_rank<2>), as the first key (G = r) and as the second one (image = G * n + r)"""
    rng = np.random.default_rng(span + 2 * nullable)
    n = 400_003
    k = _span_key(rng, n, span, nullable)
    j = rng.integers(0, 5, n).astype(np.int32)
    assert len(np.unique(np.ma.getdata(k)[~np.ma.getmaskarray(k)])) == span
    keys, by = ([k, j], ["k", "j"]) if place == "first" else ([j, k], ["j", "k"])
    run_case(dfdb_mod, ctx, keys, by, n, 51, sel_frac=0.7,
             reducers_fn=lambda v: {"si": (v["vi"], "sum"), "mf": (v["vf"], "min"), "n": (None, "count")})


@gpu
def test_image_of_two_wide_keys_stays_64_bit(dfdb_mod, ctx):
    """about 71 000 x 71 000 possible tuples among the selected rows, 2 * 10^5 present: G * n + r passes 2^32, the image column is ranked through the hash form"""
    rng = np.random.default_rng(61)
    n = 320_000
    k1 = rng.integers(0, 75_000, n).astype(np.int64)
    k2 = rng.integers(0, 75_000, n).astype(np.int64)

    def extra(t, vals, a):
        s = a < 0.7
        n1, n2 = len(np.unique(k1[s])), len(np.unique(k2[s]))
        assert n1 * n2 > 2**32 and len(np.unique(np.stack([k1[s], k2[s]], 1), axis=0)) > 190_000, (n1, n2)
    run_case(dfdb_mod, ctx, [k1, k2], ["k1", "k2"], n, 62, sel_frac=0.7, reducers_fn=lambda v: {"si": (v["vi"], "sum"), "xf": (v["vf"], "max")}, extra=extra)


@gpu
def test_a_million_hashed_keys_then_a_bool(dfdb_mod, ctx):
    rng = np.random.default_rng(63)
    n = 1_500_000
    k1 = rng.integers(0, 1_000_000, n).astype(np.int64) * 7_777_777_777          # (no dense table holds this span)
    k2 = rng.integers(0, 2, n).astype(bool)
    run_case(dfdb_mod, ctx, [k1, k2], ["k1", "k2"], n, 64, sel_frac=0.8, reducers_fn=lambda v: {"s32": (v["v32"], "sum"), "n": (None, "count")})


@gpu
def test_eight_key_columns(dfdb_mod, ctx):
    rng = np.random.default_rng(65)
    n = 150_001
    f = rng.integers(0, 3, n).astype(np.float64)
    f[rng.random(n) < 0.1] = np.nan
    f[rng.random(n) < 0.1] = -0.0
    keys = [rng.integers(-2, 2, n).astype(np.int64), rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 2, n).astype(np.uint8), rng.integers(0, 2, n).astype(bool), f,
            ["w%d" % i for i in rng.integers(0, 3, n)], np.ma.masked_array(rng.integers(0, 2, n).astype(np.int16), mask=rng.random(n) < 0.2),
            rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)]
    by = ["k%d" % i for i in range(8)]
    run_case(dfdb_mod, ctx, keys, by, n, 66)
    t9 = dfdb_mod.DFTable.from_columns({"k%d" % i: np.zeros(4, np.int64) for i in range(9)}, ctx=ctx)
    try:
        with pytest.raises(ValueError, match="1 to 8 key columns"):
            dfdb_mod.groupreduce(t9, tuple("k%d" % i for i in range(9)))
    finally:
        t9.close()


# ---------------------------------------------------------------- the accumulate pass' forms on purpose
def lds_groups(m):
    """k_group_acc_multi keeps, per group, a 4-byte count and m 8-byte accumulators in 156 KiB of a workgroup's LDS; the slot count is even"""
    return ((156 * 1024) // (4 + 8 * m)) & ~1


def acc_table(dfdb, ctx, ng, seed, reps=4):
    """ng tuples (k1 = the group, k2 = k1 % 3), every one of them among the selected rows (`keep`), rows shuffled"""
    rng = np.random.default_rng(seed)
    n = max(ng * reps, 60_000)
    i = np.arange(n)
    p = rng.permutation(n)
    k1 = (i % ng)[p].astype(np.int64) * 3 - 7
    keep = ((i // ng) % 2 == 0)[p]
    vals = {"i8": rng.integers(-128, 128, n).astype(np.int8), "u64": rng.integers(0, 2**63, n).astype(np.uint64) | np.uint64(1 << 63),
            "f32": rng.normal(0, 100, n).astype(np.float32), "vi": rng.integers(-10**15, 10**15, n).astype(np.int64), "vf": rng.normal(0, 1e3, n)}
    vals["f32"][rng.random(n) < 0.001] = np.nan
    vals["vf"][rng.random(n) < 0.02] = -0.0
    cols = {"keep": keep.astype(np.int64), "k1": k1, "k2": (k1 % 3).astype(np.int32), **vals}
    return dfdb.DFTable.from_columns(cols, block_size=65536, ctx=ctx), [k1, cols["k2"]], keep, vals


def reducers_of(m):
    if m == 16:
        r = {"%s_%s" % (st, c): (c, st) for c in ("i8", "u64", "f32") for st in ("sum", "min", "max", "mean")}
        r.update({"n": (None, "count"), "s_vf": ("vf", "sum"), "m_vi": ("vi", "min"), "x_vf": ("vf", "max")})
        return r
    return dict(list({"s_vi": ("vi", "sum"), "m_vf": ("vf", "min")}.items())[:m])


def forms_run(ctx, fn):
    """(launches of the LDS form, launches of the global form) of k_group_acc_multi while fn runs"""
    names = ("group_accumulate_multi.lds", "group_accumulate_multi.global")
    ctx.profile(True)
    before = [ctx.profile_get(k)[0] for k in names]
    try:
        fn()
    finally:
        after = [ctx.profile_get(k)[0] for k in names]
        ctx.profile(False)
    return after[0] - before[0], after[1] - before[1]


@gpu
@pytest.mark.parametrize("groups", ["1", "3", "L-1", "L", "L+1"])
@pytest.mark.parametrize("m", [0, 1, 2, 16])
def test_accumulate_forms_on_both_sides_of_the_line(dfdb_mod, ctx, m, groups):
    """exactly L(m) groups run the LDS form, L(m) + 1 (an odd count) the global one; odd counts 1, 3 and L(m) - 1 in the LDS form, whose slot count is
    (groups + 1) & ~1.  The profile notes say which form ran: a moved constant fails here instead of testing one form twice."""
    L = lds_groups(m)
    assert L == {0: 39936, 1: 13312, 2: 7986, 16: 1210}[m]
    ng = {"1": 1, "3": 3, "L-1": L - 1, "L": L, "L+1": L + 1}[groups]
    t, keys, keep, vals = acc_table(dfdb_mod, ctx, ng, 1000 * m + ng % 997)
    try:
        reds = reducers_of(m)
        assert len(reds) == m
        out = {}
        nl, ngl = forms_run(ctx, lambda: out.__setitem__("df", dfdb_mod.groupreduce(t[("keep", lambda c: c == 1), dfdb_mod.ALL], ("k1", "k2"), **reds)))
        assert len(out["df"]) == ng
        assert (nl, ngl) == ((1, 0) if ng <= L else (0, 1)), (m, ng, nl, ngl)
        check_frame(out["df"], ["k1", "k2"], keys, keep, {nm: (None if c is None else vals[c], st) for nm, (c, st) in reds.items()}, (m, groups), exact_float_sums=True)
    finally:
        t.close()


@gpu
def test_global_form_hot_slots_under_contention(dfdb_mod, ctx):
    """the global form keeps 256 LDS slots for hot groups, taken by group number mod 256: one tuple holds 30 % of the rows, and 300 tuples whose group numbers
    are the same mod 256 come in runs of 8 rows, so that a wave finds three of a kind and they contend for the hot tuple's slot"""
    rng = np.random.default_rng(71)
    ng, body = 300 * 256, 1_500_000
    head = np.arange(ng, dtype=np.int64)                                # the first ng rows number the groups: group number = key
    u = rng.random(body)
    tail = rng.integers(0, ng, body).astype(np.int64)
    tail[u < 0.3] = 17
    runs = np.repeat((17 + 256 * rng.integers(1, 300, body // 8 + 1)).astype(np.int64), 8)[:body]
    at = np.repeat(rng.random(body // 8 + 1) < 0.2, 8)[:body] & (u >= 0.3)
    tail[at] = runs[at]
    k1 = np.concatenate([head, tail])
    n = len(k1)
    keep = np.concatenate([np.ones(ng, bool), rng.random(body) < 0.9])
    vi = rng.integers(-10**15, 10**15, n).astype(np.int64)
    vf = rng.normal(0, 1e3, n)
    k2 = (k1 % 5).astype(np.int32)
    t = dfdb_mod.DFTable.from_columns({"keep": keep.astype(np.int64), "k1": k1, "k2": k2, "vi": vi, "vf": vf}, block_size=65536, ctx=ctx)
    try:
        out = {}
        reds = {"s": ("vi", "sum"), "x": ("vf", "max")}
        nl, ngl = forms_run(ctx, lambda: out.__setitem__("df", dfdb_mod.groupreduce(t[("keep", lambda c: c == 1), dfdb_mod.ALL], ("k1", "k2"), **reds)))
        assert (nl, ngl) == (0, 1) and len(out["df"]) == ng
        assert np.array_equal(out["df"]["k1"].to_numpy(), head)            # the numbering the collisions were laid out for
        assert out["df"]["count"].to_numpy()[17] > 0.25 * keep.sum()
        check_frame(out["df"], ["k1", "k2"], [k1, k2], keep, {"s": (vi, "sum"), "x": (vf, "max")}, "hot", exact_float_sums=True)
    finally:
        t.close()


@gpu
@pytest.mark.parametrize("ng", [50, 8000], ids=["lds", "global"])
def test_groups_of_negative_zero(dfdb_mod, ctx, ng):
    """a Float64 group holding only -0.0: its sum is +0.0 (the accumulators start from +0.0 as the reference's Sum() does; Julia's
    sum([-0.0]) is -0.0), its mean +0.0, its minimum and maximum -0.0; a group of -0.0 and 0.0 has minimum -0.0 and maximum 0.0"""
    t, keys, keep, vals = acc_table(dfdb_mod, ctx, ng, 80 + ng)
    t.close()
    k1 = keys[0]
    g = (k1 + 7) // 3
    vf = vals["vf"].copy()
    vf[g % 3 == 0] = -0.0
    mixed = g % 3 == 1
    vf[mixed] = np.where(np.arange(len(vf))[mixed] % 2 == 0, -0.0, 0.0)
    t = dfdb_mod.DFTable.from_columns({"keep": keep.astype(np.int64), "k1": k1, "k2": keys[1], "vf": vf}, block_size=65536, ctx=ctx)
    try:
        reds = {"s": ("vf", "sum"), "lo": ("vf", "min"), "hi": ("vf", "max"), "avg": ("vf", "mean")}
        out = {}
        nl, ngl = forms_run(ctx, lambda: out.__setitem__("df", dfdb_mod.groupreduce(t[("keep", lambda c: c == 1), dfdb_mod.ALL], ("k1", "k2"), **reds)))
        df = out["df"]
        assert (nl, ngl) == ((1, 0) if ng <= lds_groups(4) else (0, 1))
        check_frame(df, ["k1", "k2"], keys, keep, {nm: (vf, st) for nm, (_, st) in reds.items()}, "negative zero", exact_float_sums=True)
        gg = (df["k1"].to_numpy() + 7) // 3
        only, mix = gg % 3 == 0, gg % 3 == 1
        assert only.sum() > ng // 4 and mix.sum() > ng // 4
        for c in ("s", "avg"):
            v = df[c].to_numpy()
            assert np.all(v[only | mix] == 0.0) and not np.signbit(v[only | mix]).any(), c
        assert np.signbit(df["lo"].to_numpy()[only]).all() and np.signbit(df["hi"].to_numpy()[only]).all()      # (the mixed groups' signs: check_frame)
    finally:
        t.close()
