"""The yardstick of tests/test_gpu_str_pair.py pinned without a GPU: the oracle's `s1 OP s2` over two String columns equals the four-line definition on
`bytes` (str_pair_cases.cmp) for the whole content table and all six operators, a missing side gives missing, and a bare nullable predicate is refused."""
import numpy as np
import pytest

from str_pair_cases import IR_OPS, OPS, content_pairs, expect


def table(oracle, a, b, nullable=False):
    t = oracle.Table(block_size=64)
    for name, v in (("a", a), ("b", b)):
        t.add_column(name, oracle.strings_to_flat(v), dtype=oracle.NULLABLE if nullable else None)
    return t


@pytest.mark.parametrize("op", list(OPS))
def test_the_oracle_equals_the_definition_on_the_content_table(oracle, op):
    from dfdb import ir
    P = content_pairs()
    a, b = [p[0] for p in P], [p[1] for p in P]
    for x, y, l, r in ((a, b, 0, 1), (a, b, 1, 0), (a, a, 0, 0)):                    # both orders, and a column against itself
        t = table(oracle, x, y)
        cols = (x, y)
        want = np.array([expect(op, cols[l][i], cols[r][i]) for i in range(len(P))])
        got = t.view().add_predicate(IR_OPS[op](ir.col(l), ir.col(r)).to_ir()).select_indices()
        assert np.array_equal(got, np.nonzero(want)[0] + 1), op
        t.close()


def test_the_content_table_separates_the_three_outcomes():
    from str_pair_cases import cmp
    c = [cmp(a, b) for a, b in content_pairs()]
    assert c.count(-1) >= 10 and c.count(0) >= 8 and c.count(1) >= 10
    assert cmp("ÿ".encode(), b"\x7f") == 1 and cmp(b"a\0b", b"a\0c") == -1 and cmp(b"abc", b"abcdef") == -1 and cmp(b"", b"") == 0


@pytest.mark.parametrize("op", ["==", "<", ">="])
def test_a_missing_side_gives_missing_and_the_bare_predicate_is_refused(oracle, op):
    from dfdb import ir
    P = content_pairs()
    a, b = [p[0] for p in P], [p[1] for p in P]
    a[0] = None; b[3] = None; a[7] = b[7] = None
    t = table(oracle, a, b, nullable=True)
    e = IR_OPS[op](ir.col(0), ir.col(1))
    with pytest.raises(Exception, match="Bool"):
        t.view().add_predicate(e.to_ir())
    want = [expect(op, x, y) for x, y in zip(a, b)]
    got = t.view().add_predicate(ir.coalesce(e, False).to_ir()).select_indices()
    assert np.array_equal(got, np.array([i + 1 for i, w in enumerate(want) if w]))
    v = t.view()
    v.set_projection([("r", e.to_ir())])
    r = v.materialize()[0]
    assert isinstance(r, np.ma.MaskedArray)
    assert np.array_equal(np.ma.getmaskarray(r), np.array([w is None for w in want]))
    assert np.array_equal(r.compressed().astype(bool), np.array([w for w in want if w is not None]))
    t.close()
