"""tests/join_n_cases.py — the Python restatement tests/test_join_n_gpu.py compares dfdb_query_join_n with — pinned on hand-written answers (all four kinds,
"a" against "a\\0", "" against missing, NaN beside a String, a tuple whose first component matches and whose second does not, a missing value in the first, the
second and both components on each side), on tests/join_cases.py for one key and on pandas.merge(on = [..]); and the ABI surface of the entry point."""
import inspect
import os
import re

import numpy as np

import join_cases as J
import join_n_cases as JN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lists(res):
    return res[0].tolist(), res[1].tolist(), res[2]


def i64(*v):
    return np.array(v, np.int64)


def test_hand_written_answers_for_every_kind():
    # left rows 1..5: (7,1) (7,2) (3,1) (9,9) (5,0) ; right rows 1..6: (5,0) (7,2) (8,1) (7,2) (5,0) (7,1)
    L = [(i64(7, 7, 3, 9, 5), None), (i64(1, 2, 1, 9, 0), None)]
    R = [(i64(5, 7, 8, 7, 5, 7), None), (i64(0, 2, 1, 2, 0, 1), None)]
    assert lists(JN.join_n_ref(L, None, R, None, "inner")) == ([1, 2, 2, 5, 5], [6, 2, 4, 1, 5], (5, 6, 0, 0))
    assert lists(JN.join_n_ref(L, None, R, None, "left")) == ([1, 2, 2, 3, 4, 5, 5], [6, 2, 4, 0, 0, 1, 5], (5, 6, 0, 0))
    assert lists(JN.join_n_ref(L, None, R, None, "semi")) == ([1, 2, 5], [6, 2, 1], (5, 6, 0, 0))
    assert lists(JN.join_n_ref(L, None, R, None, "anti")) == ([3, 4], [0, 0], (5, 6, 0, 0))
    # selections and row bases: left rows 2, 5 (0-based 1, 4), right rows 1, 4 (0-based 0, 3)
    assert lists(JN.join_n_ref(L, [1, 4], R, [0, 3], "left", lbase=100, rbase=1000)) == ([102, 105], [1004, 1001], (2, 2, 0, 0))


def test_the_first_component_matches_and_the_second_does_not():
    L = [(i64(4, 4), None), (i64(1, 2), None)]
    R = [(i64(4, 4, 4), None), (i64(2, 3, 2), None)]
    assert lists(JN.join_n_ref(L, None, R, None, "inner")) == ([2, 2], [1, 3], (2, 3, 0, 0))
    assert lists(JN.join_n_ref(L, None, R, None, "anti")) == ([1], [0], (2, 3, 0, 0))
    # and the components do not trade places: (1, 2) is not (2, 1)
    assert lists(JN.join_n_ref([(i64(1), None), (i64(2), None)], None, [(i64(2), None), (i64(1), None)], None, "inner")) == ([], [], (1, 1, 0, 0))


def test_strings_compare_by_bytes_and_length():
    L = [(["a", "a\0", "", None, "ab"], None)]
    R = [(["a\0", "a", None, "", "a", "abc"], None)]
    # "a" and "a\0" differ; "" matches "" and not a missing row; missing matches nothing, a missing row included
    assert lists(JN.join_n_ref(L, None, R, None, "inner")) == ([1, 1, 2, 3], [2, 5, 1, 4], (5, 6, 1, 1))
    assert lists(JN.join_n_ref(L, None, R, None, "left")) == ([1, 1, 2, 3, 4, 5], [2, 5, 1, 4, 0, 0], (5, 6, 1, 1))
    assert lists(JN.join_n_ref(L, None, R, None, "semi")) == ([1, 2, 3], [2, 1, 4], (5, 6, 1, 1))
    assert lists(JN.join_n_ref(L, None, R, None, "anti")) == ([4, 5], [0, 0], (5, 6, 1, 1))
    assert JN.join_n_ref([([b"a\x00b"], None)], None, [([b"a\x00b", b"a\x00c", b"a"], None)], None, "inner")[1].tolist() == [1]


def test_nan_beside_a_string():
    nan2 = np.array([0x7ff8000000000001], np.uint64).view(np.float64)[0]
    L = [(np.array([np.nan, np.nan, -0.0, 0.0]), None), (["x", "y", "z", "z"], None)]
    R = [(np.array([nan2, 0.0, -0.0, np.nan]), None), (["x", "z", "z", "x"], None)]
    # every NaN is one key, -0.0 and 0.0 are two
    assert lists(JN.join_n_ref(L, None, R, None, "inner")) == ([1, 1, 3, 4], [1, 4, 3, 2], (4, 4, 0, 0))
    assert lists(JN.join_n_ref(L, None, R, None, "anti")) == ([2], [0], (4, 4, 0, 0))


def test_a_missing_component_matches_nothing():
    # the bytes under a missing flag would match if they were read
    lm0, lm1 = np.array([True, False, True, False]), np.array([False, True, True, False])
    L = [(i64(1, 1, 1, 1), lm0), (i64(2, 2, 2, 2), lm1)]                                   # left row 1: first missing, 2: second, 3: both, 4: none
    R = [(i64(1, 1, 1, 1), lm0), (i64(2, 2, 2, 2), lm1)]
    assert lists(JN.join_n_ref(L, None, R, None, "inner")) == ([4], [4], (4, 4, 3, 3))   # a row with both components missing is counted once
    assert lists(JN.join_n_ref(L, None, R, None, "left")) == ([1, 2, 3, 4], [0, 0, 0, 4], (4, 4, 3, 3))
    assert lists(JN.join_n_ref(L, None, R, None, "anti")) == ([1, 2, 3], [0, 0, 0], (4, 4, 3, 3))
    plain = [(i64(1, 1, 1, 1), None), (i64(2, 2, 2, 2), None)]
    assert lists(JN.join_n_ref(L, None, plain, None, "semi")) == ([4], [1], (4, 4, 3, 0))
    assert lists(JN.join_n_ref(plain, None, R, None, "inner")) == ([1, 2, 3, 4], [4, 4, 4, 4], (4, 4, 0, 3))
    # a missing String (None) beside a live number; a missing row outside the selection is not counted
    S = [(i64(5, 5), None), ([None, "k"], None)]
    assert lists(JN.join_n_ref(S, None, S, None, "inner")) == ([2], [2], (2, 2, 1, 1))
    assert JN.join_n_ref(S, [1], S, [1], "inner")[2] == (1, 1, 0, 0)


def test_one_key_is_join_cases():
    rng = np.random.default_rng(4)
    for dt in J.EDGE_DTYPES:
        left, right = J.edge_sides(dt, 120, 90)
        lm, rm = rng.random(120) < 0.2, rng.random(90) < 0.2
        lrows, rrows = np.flatnonzero(rng.random(120) < 0.7), np.flatnonzero(rng.random(90) < 0.7)
        want = J.join_ref_all(left, lm, lrows, right, rm, rrows, 10, 20)
        got = JN.join_n_ref_all([(left, lm)], lrows, [(right, rm)], rrows, 10, 20)
        for kind in J.KINDS:
            assert lists(got[kind]) == lists(want[kind]), (dt, kind)


def test_against_pandas_merge_on_several_columns():
    import pandas as pd
    rng = np.random.default_rng(21)
    names = ["ab", "a", "", "abcdefgh", "abcdefghi", "żółw"]
    for nl, nr, hi in ((60, 50, 4), (300, 200, 9), (1, 1, 1)):
        la, lb, ls = rng.integers(0, hi, nl).astype(np.int64), rng.integers(0, 3, nl).astype(np.int32), [names[i] for i in rng.integers(0, len(names), nl)]
        ra, rb, rs = rng.integers(0, hi, nr).astype(np.int64), rng.integers(0, 3, nr).astype(np.int32), [names[i] for i in rng.integers(0, len(names), nr)]
        left = pd.DataFrame({"a": la, "b": lb, "s": ls, "l": np.arange(1, nl + 1)})
        right = pd.DataFrame({"a": ra, "b": rb, "s": rs, "r": np.arange(1, nr + 1)})
        for on, lc, rc in ((["a", "b"], [(la, None), (lb, None)], [(ra, None), (rb, None)]), (["s", "a"], [(ls, None), (la, None)], [(rs, None), (ra, None)]),
                           (["a", "s", "b"], [(la, None), (ls, None), (lb, None)], [(ra, None), (rs, None), (rb, None)])):
            for how in ("inner", "left"):
                m = left.merge(right, on=on, how=how, sort=False)
                gl, gr, info = JN.join_n_ref(lc, None, rc, None, how)
                assert info == (nl, nr, 0, 0)
                assert m["l"].tolist() == gl.tolist() and m["r"].fillna(0).astype(np.int64).tolist() == gr.tolist(), (nl, nr, on, how)


def test_generators_are_what_their_names_say():
    pool = JN.string_pool()
    assert len(set(pool)) == len(pool) and {len(s) for s in pool} >= set(JN.STRING_LENGTHS)
    assert JN.chunks_of(pool) == 32 and JN.chunks_of([b"", None]) == 0 and JN.chunks_of([b"123456789"]) == 2
    left, right = JN.string_sides(500, 400)
    semi, anti = JN.join_n_ref([(left, None)], None, [(right, None)], None, "semi"), JN.join_n_ref([(left, None)], None, [(right, None)], None, "anti")
    assert len(semi[0]) and len(anti[0]) and len(semi[0]) + len(anti[0]) == 500
    (l0, l1), (r0, r1) = JN.pair_sides(300, 200)
    first_only = np.isin(l0, r0) & ~np.array([k in set(zip(r0.tolist(), r1.tolist())) for k in zip(l0.tolist(), l1.tolist())])
    assert first_only.any()
    assert JN.with_missing(["a", "b"], [True, False]) == [None, "b"]


def test_the_abi_declares_lists_and_exports_the_entry_point():
    import ctypes
    import dfdb
    text = open(os.path.join(ROOT, "include", "dfdb.h")).read()
    decl = re.search(r"^int32_t dfdb_query_join_n\(([^;]*)\);", text, re.M | re.S)
    assert decl and len(decl.group(1).split(",")) == 8, decl
    assert re.search(r"DFDB_JOIN_MAX_KEYS = 8\b", text)
    assert "dfdb_query_join_n" in dfdb.SYMBOLS
    fn = getattr(dfdb.load(), "dfdb_query_join_n")
    assert isinstance(fn, ctypes._CFuncPtr) and len(fn.argtypes) == 8
    from dfdb.api import _Query
    assert list(inspect.signature(_Query.join_count_n).parameters)[:5] == ["self", "other", "cols", "other_cols", "kind"]
