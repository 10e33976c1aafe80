"""`s == "c"`, `s != "c"`, startswith(s, "c") and endswith(s, "c") over a flat String column in every compiled form: k_str_match_short staged through LDS and
with direct probes, with one probe and with two, capturing the selected rows or not, over a fresh mask and AND-ed into one; k_str_match above 64 bytes; the
gathers behind them.  The yardstick is the oracle through helpers (count, bitmap, indices and materialized columns bit for bit) and, beside it, the
definition on `bytes` (str_match_cases.expect); tests/test_str_match_cpu.py pins the two together and shows that every column here decides its case.  The
form that ran is read from the profile: `str_match.staged` / `.direct` / `.long` are noted by run_str_step."""
import numpy as np
import pytest

import str_match_cases as M
from helpers import apply_stages, assert_same
from str_match_cases import BUILDERS, EDGE_LEADS, EDGE_LENGTHS, EDGE_TOTALS, MODES, PATTERN_LENGTHS, SIZES, S, build

pytestmark = pytest.mark.gpu

BS = 65536
FORMS = ("str_match.staged", "str_match.direct", "str_match.long")
NAMES = FORMS + ("str_match", "str_compact_captured", "fill_const_strings", "str_gather_bytes", "dict_scan", "interp_predicate", "jit_predicate")


def make(oracle, dfdb_mod, ctx, rows, kind="plain", **kw):
    p = build(oracle, dfdb_mod, {"s": S(rows, kind == "nullable"), "a": np.arange(len(rows), dtype=np.int64)}, ctx=ctx, **kw)
    if kind == "dict":
        assert p.d.build_dictionary("s", 65535) == len(set(rows))
    return p


@pytest.fixture(scope="module")
def tables(oracle, dfdb_mod, ctx):
    """(builder, pattern length, rows, kind) -> the table pair, its values and its tile byte totals; kind: plain, nullable (every 7th row missing), dict"""
    made = {}

    def get(builder, L, n, kind="plain"):
        key = (builder, L, n, kind)
        if key not in made:
            rows, _ = BUILDERS[builder](n, M.pattern(L))
            if kind == "nullable":
                rows = M.with_missing(rows)
            made[key] = (make(oracle, dfdb_mod, ctx, rows, kind, block_size=BS), rows, M.tile_totals(rows))
        return made[key]
    yield get
    for p, _, _ in made.values():
        p.d.close()
        p.o.close()


def run(ctx, p, stages, proj):
    """the view equals the oracle's in every observable; returns the oracle's view and the launches by profile name meanwhile"""
    ov, dv = apply_stages(p, stages, proj=proj)
    ctx.profile(True)
    before = [ctx.profile_get(k)[0] for k in NAMES]
    try:
        assert_same(p, ov, dv)
    finally:
        after = [ctx.profile_get(k)[0] for k in NAMES]
        ctx.profile(False)
    return ov, {k: a - b for k, a, b in zip(NAMES, after, before)}


def assert_expected(ov, names, rows, ids):
    """the oracle's materialized columns are the rows the definition selects: `a` holds each row's own number, `s` its bytes"""
    assert ov.nrow() == len(ids)
    for name, col in zip(names, ov.materialize()):
        if name == "a":
            assert np.array_equal(col, ids)
        else:
            want = [rows[i] for i in ids]
            assert np.array_equal(col[0], [len(v) for v in want]) and col[1].tobytes() == b"".join(want)


def assert_route(n, kind, form, mode, L, rows, ids, whole_query):
    """n: launches by name.  The match ran in the form the column's tile totals and the pattern's length select, nothing fell to the interpreter, and the
    projection of `s` took the route the plan gives it.  whole_query: the match is the query's only stage and only step"""
    assert n["interp_predicate"] + n["jit_predicate"] == 0, n
    if kind == "dict":
        assert n["dict_scan"] >= 1 and n["str_match"] == 0 and not any(n[f] for f in FORMS), n
        return
    assert n["str_match"] >= 1 and n["dict_scan"] == 0 and n["str_match." + form] == n["str_match"], n
    assert all(n[f] == 0 for f in FORMS if f != "str_match." + form), n
    if len(ids) == 0:
        return
    some_bytes = any(len(rows[i]) for i in ids)
    if kind == "nullable" or not whole_query:
        assert n["str_compact_captured"] == 0, n                            # CAP is the whole query's only step over a plain column
        if kind == "nullable":
            assert n["fill_const_strings"] == 0 and (n["str_gather_bytes"] >= 1) == some_bytes, n
    elif mode == "==":
        assert n["fill_const_strings"] >= 1 and n["str_compact_captured"] == 0 and n["str_gather_bytes"] == 0, n       # every selected row holds the constant
    elif L <= 64:
        assert n["str_compact_captured"] >= 1 and n["str_gather_bytes"] == 0 and n["fill_const_strings"] == 0, n       # CAP: the match pass kept the rows
    else:
        assert n["str_compact_captured"] == 0 and n["fill_const_strings"] == 0 and (n["str_gather_bytes"] >= 1) == some_bytes, n   # above 64 bytes: K6


def predicate(mode, pat, kind):
    from dfdb import ir
    e = M.term(mode, ir.col(0), pat)
    return ir.coalesce(e, False) if kind == "nullable" else e


# ---------------------------------------------------------------- every form
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", PATTERN_LENGTHS)
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_every_form(ctx, tables, builder, L, mode):
    from dfdb import ir
    pat = M.pattern(L)
    Sc, A = ir.col(0), ir.col(1)
    for n in SIZES:
        p, rows, totals = tables(builder, L, n)
        form = M.form(L, totals)
        assert form == ("long" if L > 64 else "direct" if L == 0 or (builder == "dense" and n > 1) else "staged")
        pred = predicate(mode, pat, "plain")
        hit = M.selected(mode, rows, pat)
        # (a) the only predicate, the whole table projected
        ov, ln = run(ctx, p, [("pred", pred)], None)
        assert_expected(ov, "sa", rows, hit)
        assert np.array_equal(ov.select_indices(), hit + 1)
        assert_route(ln, "plain", form, mode, L, rows, hit, True)
        # (b) after a range stage that leaves whole tiles empty and cuts one in half: AND-ed into the mask, the dead tiles skipped
        lo = n * 3 // 10 + 1
        hi = max(lo, n * 4 // 5)
        ids = hit[(hit >= lo - 1) & (hit <= hi - 1)]
        ov, ln = run(ctx, p, [("range", lo, 1, hi), ("pred", pred)], None)
        assert_expected(ov, "sa", rows, ids)
        assert_route(ln, "plain", form, mode, L, rows, ids, False)
        # (c) the second conjunct beside a term over the Int64 column
        ids = hit[hit > n // 3]
        ov, ln = run(ctx, p, [("pred", (A > n // 3) & pred)], None)
        assert_expected(ov, "sa", rows, ids)
        assert_route(ln, "plain", form, mode, L, rows, ids, False)
        # (d) the only stage, the String column projected alone and beside the Int64 column
        for names, proj in (("s", [("s", Sc)]), ("sa", [("s", Sc), ("a", A)])):
            ov, ln = run(ctx, p, [("pred", pred)], proj)
            assert_expected(ov, names, rows, hit)
            assert_route(ln, "plain", form, mode, L, rows, hit, True)


# ---------------------------------------------------------------- the staging arithmetic at its edges
@pytest.mark.parametrize("lead", EDGE_LEADS)
@pytest.mark.parametrize("total", EDGE_TOTALS)
@pytest.mark.parametrize("L", EDGE_LENGTHS)
def test_edges(oracle, dfdb_mod, ctx, L, total, lead):
    """a tile of exactly 8144 / 8145 bytes at an arena offset of 0, 1 and 15 (mod 16), matching rows at its first and last position and at the table's end"""
    from dfdb import ir
    pat = M.pattern(L)
    rows, totals = M.edge(total, lead, pat)
    form = "staged" if total == M.STAGE_MAX else "direct"
    assert M.form(L, totals) == form
    p = make(oracle, dfdb_mod, ctx, rows, block_size=BS)
    try:
        for mode in MODES:
            hit = M.selected(mode, rows, pat)
            ov, ln = run(ctx, p, [("pred", predicate(mode, pat, "plain"))], [("s", ir.col(0))])
            assert_expected(ov, "s", rows, hit)
            assert np.array_equal(ov.select_indices(), hit + 1)
            assert_route(ln, "plain", form, mode, L, rows, hit, True)
            lo, hi = M.TILE + 1, 2 * M.TILE                                      # tile 1 alone alive: AND_EXISTING over the edge tile, dead tiles around it
            ids = hit[(hit >= lo - 1) & (hit <= hi - 1)]
            ov, ln = run(ctx, p, [("range", lo, 1, hi), ("pred", predicate(mode, pat, "plain"))], [("s", ir.col(0))])
            assert_expected(ov, "s", rows, ids)
            assert_route(ln, "plain", form, mode, L, rows, ids, False)
    finally:
        p.d.close()
        p.o.close()


# ---------------------------------------------------------------- the same answers by other routes
@pytest.mark.parametrize("kind", ["nullable", "dict"])
@pytest.mark.parametrize("L", PATTERN_LENGTHS)
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_other_routes(ctx, tables, builder, L, kind):
    """Union{String,Missing} with every 7th row missing, queried as coalesce(term, false): CAP must not run and the missing rows ride the gather.  And with a
    dictionary built: K9's LUT scan answers."""
    from dfdb import ir
    pat = M.pattern(L)
    for n in SIZES:
        p, rows, totals = tables(builder, L, n, kind)
        form = M.form(L, totals)
        for mode in MODES:
            pred = predicate(mode, pat, kind)
            hit = M.selected(mode, rows, pat)
            ov, ln = run(ctx, p, [("pred", pred)], None)
            assert_expected(ov, "sa", rows, hit)
            assert np.array_equal(ov.select_indices(), hit + 1)
            assert_route(ln, kind, form, mode, L, rows, hit, True)
            ov, ln = run(ctx, p, [("pred", pred)], [("s", ir.col(0))])
            assert ov.nrow() == len(hit)
            assert_route(ln, kind, form, mode, L, rows, hit, True)
        if kind == "nullable":                                                   # the missing rows themselves: projected through the ordinary gather
            ov, ln = run(ctx, p, [("range", 1, 1, n)], [("s", ir.col(0))])
            sizes = ov.materialize()[0][0]
            assert np.array_equal(sizes, [-1 if v is None else len(v) for v in rows])


# ---------------------------------------------------------------- through files
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_through_files_and_the_block_stream(oracle, dfdb_mod, ctx, tmp_path, builder):
    """the oracle's writer (liblz4) wrote the table: resident after the device LZ4 decode, and block-streamed in chunks of 3 blocks of 600 rows — a chunk
    boundary every 1800 rows, inside a 1024-row tile of the resident column; a chunk is a table of its own with its own tile totals"""
    from dfdb import ir
    L, n = 17, SIZES[-1]
    pat = M.pattern(L)
    rows, totals = BUILDERS[builder](n, pat)
    path = str(tmp_path / "tb")
    p = make(oracle, dfdb_mod, ctx, rows, block_size=600, via_files=path)
    lazy = dfdb_mod.open_table(path, load=False, ctx=ctx)
    try:
        for mode in MODES:
            pred = predicate(mode, pat, "plain")
            hit = M.selected(mode, rows, pat)
            ov, ln = run(ctx, p, [("pred", pred)], None)
            assert_expected(ov, "sa", rows, hit)
            assert_route(ln, "plain", M.form(L, totals), mode, L, rows, hit, True)
            with dfdb_mod.stream(dfdb_mod.DFView(lazy)[pred, ["s", "a"]], 3) as st:
                parts = [(part.indices(), part.materialize()) for part in st]
            assert len(parts) >= 2                                               # the table did not fit one chunk
            assert np.array_equal(np.concatenate([i for i, _ in parts]), hit + 1)
            assert np.array_equal(np.concatenate([m[1] for _, m in parts]), hit)
            assert np.array_equal(np.concatenate([m[0][0] for _, m in parts]), [len(rows[i]) for i in hit])
            assert b"".join(m[0][1].tobytes() for _, m in parts) == b"".join(rows[i] for i in hit)
    finally:
        lazy.close()
        p.d.close()
        p.o.close()
