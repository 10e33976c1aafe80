"""The yardstick of tests/test_gpu_str_match.py pinned without a GPU: the oracle's `s OP "const"` (==, !=, startswith, endswith) equals the definition on
`bytes` (str_match_cases.expect) for every pattern length, mode and column builder; every committed input decides its case (the expected selection is
neither empty nor everything); and the builders' own conditions hold — tile byte totals, the arena offset of the edge tile, staged or direct."""
import numpy as np
import pytest

import str_match_cases as M
from str_match_cases import BUILDERS, EDGE_LEADS, EDGE_LENGTHS, EDGE_TOTALS, MODES, PATTERN_LENGTHS, SIZES, STAGE_MAX


def oracle_indices(oracle, rows, mode, pat):
    from dfdb import ir
    nullable = any(v is None for v in rows)
    t = oracle.Table(block_size=4096)
    t.add_column("s", oracle.strings_to_flat(rows), dtype=oracle.NULLABLE if nullable else None)
    e = M.term(mode, ir.col(0), pat)
    v = t.view().add_predicate((ir.coalesce(e, False) if nullable else e).to_ir())
    got, n = v.select_indices(), v.nrow()
    t.close()
    return got, n


@pytest.mark.parametrize("L", PATTERN_LENGTHS)
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_the_oracle_equals_the_definition(oracle, builder, L):
    pat = M.pattern(L)
    for n in (65, SIZES[-1]):
        rows, _ = BUILDERS[builder](n, pat)
        for col in (rows, M.with_missing(rows)):
            for mode in MODES:
                got, cnt = oracle_indices(oracle, col, mode, pat)
                want = M.selected(mode, col, pat) + 1
                assert cnt == len(want) and np.array_equal(got, want), (builder, L, n, mode)


@pytest.mark.parametrize("L", EDGE_LENGTHS)
def test_the_oracle_equals_the_definition_on_the_edge_tables(oracle, L):
    pat = M.pattern(L)
    for total in EDGE_TOTALS:
        for lead in EDGE_LEADS:
            rows, _ = M.edge(total, lead, pat)
            for mode in MODES:
                got, cnt = oracle_indices(oracle, rows, mode, pat)
                want = M.selected(mode, rows, pat) + 1
                assert cnt == len(want) and np.array_equal(got, want), (L, total, lead, mode)


def test_the_patterns_put_distinct_bytes_where_the_kernels_decide():
    for L in PATTERN_LENGTHS:
        pat = M.pattern(L)
        assert len(pat) == L
        at = sorted({i for i in M.DECIDING + (L - 1,) if 0 <= i < L})
        assert len({pat[i] for i in at}) == len(at), L
        if L >= 2:
            assert 0 in pat and max(pat) >= 0x80
        V = M.variants(pat)
        assert V[0] == pat and len(set(V)) == len(V) and b"" in V and pat + pat in V
        if L:
            same_len = [v for v in V if len(v) == L and v != pat]
            differ_at = sorted(next(i for i in range(L) if v[i] != pat[i]) for v in same_len)
            assert differ_at == at and all(sum(a != b for a, b in zip(v, pat)) == 1 for v in same_len), L
            assert {pat + b"x", b"x" + pat, pat[:-1]} <= set(V)
    assert all(len(f) <= 3 for f in M.FILL)


@pytest.mark.parametrize("L", PATTERN_LENGTHS)
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_every_committed_column_decides_its_case_and_takes_its_form(builder, L):
    pat = M.pattern(L)
    for n in SIZES:
        rows, totals = BUILDERS[builder](n, pat)
        assert len(rows) == n and totals == M.tile_totals(rows)
        # a variant at the first and last row of every tile and of the table, the variants off the 64-row boundaries
        V = set(M.variants(pat))
        for t in range(0, n, M.TILE):
            assert rows[t] in V and rows[min(t + M.TILE, n) - 1] in V
        assert rows[-1] == pat
        if builder == "lean":
            assert all(rows[i] in V for i in range(3, n, 16) if i % M.TILE not in (0, M.TILE - 1) and i != n - 1) and 3 % 64 != 0
            assert all(len(v) <= 3 or v in V for v in rows)
        nullable = M.with_missing(rows)
        ntotals = M.tile_totals(nullable)
        for col, tot in ((rows, totals), (nullable, ntotals)):
            # the form, from the host's totals and the launcher's rule: lean is staged, dense direct (n = 1 cannot exceed the threshold), above 64 bytes neither
            want = "long" if L > 64 else "direct" if L == 0 or (builder == "dense" and n > 1) else "staged"
            assert M.form(L, tot) == want, (builder, L, n, max(tot))
            if n > 1 or col is rows:
                for mode in MODES:
                    M.assert_decides(mode, col, pat)


@pytest.mark.parametrize("L", EDGE_LENGTHS)
def test_the_edge_tables_sit_on_either_side_of_the_threshold(L):
    pat = M.pattern(L)
    for lead in EDGE_LEADS:
        below, tb = M.edge(STAGE_MAX, lead, pat)
        above, ta = M.edge(STAGE_MAX + 1, lead, pat)
        assert M.form(L, tb) == "staged" and M.form(L, ta) == "direct"
        assert tb[0] % 16 == lead and ta[0] % 16 == lead and tb[1] == STAGE_MAX and ta[1] == STAGE_MAX + 1
        assert sum(a != b for a, b in zip(below, above)) == 1                  # one row, one byte longer
        for rows in (below, above):
            assert len(rows) == 2 * M.TILE + 300
            for mode in MODES:
                M.assert_decides(mode, rows, pat)
            # the matching rows at the tile's two ends, and the table's last row
            assert M.expect("endswith", rows[M.TILE], pat) and not M.expect("==", rows[M.TILE], pat)
            assert all(M.expect(m, rows[2 * M.TILE - 1], pat) for m in ("==", "startswith", "endswith")) and rows[-1] == pat
