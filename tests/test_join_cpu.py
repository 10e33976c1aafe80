"""tests/join_cases.py — the numpy restatement tests/test_join_gpu.py compares the device join with — pinned on hand-written answers (all four kinds,
duplicates on both sides, NaN against NaN, -0.0 against 0.0, a missing row on either side, an empty side) and on pandas.merge for integer keys; and the ABI
surface of the join: the header declares both entry points, dfdb.SYMBOLS lists them and the built library exports them."""
import os
import re

import numpy as np

import join_cases as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lists(res):
    return res[0].tolist(), res[1].tolist(), res[2]


def test_hand_written_answers_for_every_kind():
    # left rows 1..5: 7 7 3 9 5 ; right rows 1..6: 5 7 8 7 5 5
    L = np.array([7, 7, 3, 9, 5], np.int64)
    R = np.array([5, 7, 8, 7, 5, 5], np.int64)
    assert lists(J.join_ref(L, None, None, R, None, None, "inner")) == ([1, 1, 2, 2, 5, 5, 5], [2, 4, 2, 4, 1, 5, 6], (5, 6, 0, 0))
    assert lists(J.join_ref(L, None, None, R, None, None, "left")) == ([1, 1, 2, 2, 3, 4, 5, 5, 5], [2, 4, 2, 4, 0, 0, 1, 5, 6], (5, 6, 0, 0))
    assert lists(J.join_ref(L, None, None, R, None, None, "semi")) == ([1, 2, 5], [2, 2, 1], (5, 6, 0, 0))
    assert lists(J.join_ref(L, None, None, R, None, None, "anti")) == ([3, 4], [0, 0], (5, 6, 0, 0))


def test_selections_and_row_bases():
    L = np.array([7, 7, 3, 9, 5], np.int64)
    R = np.array([5, 7, 8, 7, 5, 5], np.int64)
    # left rows 2, 4, 5 (0-based 1, 3, 4), right rows 1, 4, 6 (0-based 0, 3, 5); bases 100 and 1000
    got = J.join_ref(L, None, [1, 3, 4], R, None, [0, 3, 5], "left", lbase=100, rbase=1000)
    assert lists(got) == ([102, 104, 105, 105], [1004, 0, 1001, 1006], (3, 3, 0, 0))
    got = J.join_ref(L, None, [1, 3, 4], R, None, [0, 3, 5], "anti", lbase=100, rbase=1000)
    assert lists(got) == ([104], [0], (3, 3, 0, 0))


def test_floats_compare_with_isequal():
    nan2 = np.array([0x7ff8000000000001], np.uint64).view(np.float64)[0]
    nneg = np.array([0xfff8000000000dea], np.uint64).view(np.float64)[0]
    L = np.array([np.nan, -0.0, 0.0, np.inf, 1.5])
    R = np.array([nneg, 0.0, nan2, -np.inf, -0.0, -0.0])
    # every NaN is one key; -0.0 and 0.0 are two
    assert lists(J.join_ref(L, None, None, R, None, None, "inner")) == ([1, 1, 2, 2, 3], [1, 3, 5, 6, 2], (5, 6, 0, 0))
    assert lists(J.join_ref(L, None, None, R, None, None, "anti")) == ([4, 5], [0, 0], (5, 6, 0, 0))
    L32, R32 = L.astype(np.float32), R.astype(np.float32)
    assert lists(J.join_ref(L32, None, None, R32, None, None, "semi")) == ([1, 2, 3], [1, 5, 2], (5, 6, 0, 0))


def test_a_missing_key_matches_nothing():
    L = np.array([4, 4, 6], np.int64)
    R = np.array([4, 6, 4], np.int64)
    lm = np.array([False, True, False])
    rm = np.array([False, True, False])
    # left row 2 is missing (its bytes say 4), right row 2 is missing (its bytes say 6)
    assert lists(J.join_ref(L, lm, None, R, rm, None, "inner")) == ([1, 1], [1, 3], (3, 3, 1, 1))
    assert lists(J.join_ref(L, lm, None, R, rm, None, "left")) == ([1, 1, 2, 3], [1, 3, 0, 0], (3, 3, 1, 1))
    assert lists(J.join_ref(L, lm, None, R, rm, None, "semi")) == ([1], [1], (3, 3, 1, 1))
    assert lists(J.join_ref(L, lm, None, R, rm, None, "anti")) == ([2, 3], [0, 0], (3, 3, 1, 1))
    # missing against missing: nothing
    assert lists(J.join_ref(L, np.ones(3, bool), None, R, np.ones(3, bool), None, "inner")) == ([], [], (3, 3, 3, 3))
    # a missing row outside the selection is not counted
    assert J.join_ref(L, lm, [0, 2], R, rm, [0, 2], "inner")[2] == (2, 2, 0, 0)


def test_an_empty_side():
    L = np.array([1, 2], np.int64)
    E = np.zeros(0, np.int64)
    for kind, want in (("inner", ([], [])), ("left", ([1, 2], [0, 0])), ("semi", ([], [])), ("anti", ([1, 2], [0, 0]))):
        assert lists(J.join_ref(L, None, None, E, None, None, kind)) == want + ((2, 0, 0, 0),)
        assert lists(J.join_ref(E, None, None, L, None, None, kind)) == ([], [], (0, 2, 0, 0))
        assert lists(J.join_ref(L, None, [], L, None, None, kind)) == ([], [], (0, 2, 0, 0))


def test_against_pandas_merge_for_integer_keys():
    import pandas as pd
    rng = np.random.default_rng(20)
    for nl, nr, hi in ((50, 40, 12), (200, 300, 40), (300, 5, 3), (1, 1, 1)):
        L = rng.integers(0, hi, nl).astype(np.int64)
        R = rng.integers(0, hi, nr).astype(np.int64)
        left = pd.DataFrame({"k": L, "l": np.arange(1, nl + 1)})
        right = pd.DataFrame({"k": R, "r": np.arange(1, nr + 1)})
        for how in ("inner", "left"):
            # pandas keeps the left order, and the right order within a key; rows are given in row order
            m = left.merge(right, on="k", how=how, sort=False)
            gl, gr, info = J.join_ref(L, None, None, R, None, None, how)
            assert info == (nl, nr, 0, 0)
            assert m["l"].tolist() == gl.tolist(), (nl, nr, how)
            assert m["r"].fillna(0).astype(np.int64).tolist() == gr.tolist(), (nl, nr, how)
        has = np.isin(L, R)
        assert J.join_ref(L, None, None, R, None, None, "semi")[0].tolist() == (np.flatnonzero(has) + 1).tolist()
        assert J.join_ref(L, None, None, R, None, None, "anti")[0].tolist() == (np.flatnonzero(~has) + 1).tolist()


def test_generators_are_what_their_names_say():
    r = J.unique_keys(1025)
    assert len(np.unique(r)) == 1025
    p = J.probe_keys(4097, r)
    assert p[0] < r.min() and p[1] > r.max() and np.isin(p, r).any() and (~np.isin(p, r)).any()
    for dt in J.EDGE_DTYPES:
        a, b = J.edge_sides(dt)
        assert a.dtype == np.dtype(dt) and b.dtype == np.dtype(dt)
        gl, _, _ = J.join_ref(a, None, None, b, None, None, "semi")
        ga, _, _ = J.join_ref(a, None, None, b, None, None, "anti")
        assert len(gl) and len(ga) and len(gl) + len(ga) == len(a), dt
    x, m = J.nullable_side(1000, 3)
    assert m.sum() == 200


def test_the_abi_declares_lists_and_exports_the_join():
    import ctypes
    import dfdb
    text = open(os.path.join(ROOT, "include", "dfdb.h")).read()
    for name in ("dfdb_query_join", "dfdb_query_join_fetch"):
        assert re.search(r"^int32_t %s\(" % name, text, re.M), name
        assert name in dfdb.SYMBOLS
        assert isinstance(getattr(dfdb.load(), name), ctypes._CFuncPtr)
    for k, v in (("INNER", 0), ("LEFT", 1), ("SEMI", 2), ("ANTI", 3)):
        assert re.search(r"DFDB_JOIN_%s = %d\b" % (k, v), text) and getattr(dfdb, "JOIN_" + k) == v
    for name in ("join_rows", "innerjoin", "semijoin", "antijoin"):
        assert callable(getattr(dfdb, name))
