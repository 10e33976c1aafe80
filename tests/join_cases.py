"""What dfdb_query_join / dfdb_query_join_fetch must answer, restated in numpy, and the columns tests/test_join_gpu.py runs (tests/test_join_cpu.py pins this
file on hand-written answers and on pandas.merge).

Keys compare with isequal: two values are one key when their order images (tests/order_stat_cases.py `image`: every NaN one value, -0.0 and 0.0 two, integers
by value) are equal.  A row whose key is missing matches nothing.  The result is two parallel lists of 1-based table rows, ordered by left row and within one
left row by right row; right row 0 = no match."""
import numpy as np

import order_stat_cases as K

KINDS = ("inner", "left", "semi", "anti")
KIND_CODE = {"inner": 0, "left": 1, "semi": 2, "anti": 3}


def _side(keys, miss, rows):
    k = np.ascontiguousarray(keys)
    m = np.zeros(len(k), bool) if miss is None else np.asarray(miss, bool)
    r = np.arange(len(k), dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    return K.image(k) if len(k) else np.zeros(0, np.uint64), m, r


def join_ref(lkeys, lmiss, lrows, rkeys, rmiss, rrows, kind, lbase=0, rbase=0):
    """(left_rows, right_rows, info[0:4]) by brute force: for every selected left row, ascending, every selected right row, ascending, is compared with it.
    lrows / rrows: the 0-based selected rows, ascending (None: all); lmiss / rmiss: missing flags (None: none); lbase / rbase: the tables' row bases"""
    assert kind in KINDS
    return join_ref_all(lkeys, lmiss, lrows, rkeys, rmiss, rrows, lbase, rbase, (kind,))[kind]


def join_ref_all(lkeys, lmiss, lrows, rkeys, rmiss, rrows, lbase=0, rbase=0, kinds=KINDS):
    """kind -> join_ref's answer, every kind from ONE pass of comparisons"""
    limg, lm, lr = _side(lkeys, lmiss, lrows)
    rimg, rm, rr = _side(rkeys, rmiss, rrows)
    rr_live = rr[~rm[rr]] if len(rr) else rr                    # ascending: so is every left row's list of matches
    rk_live = rimg[rr_live] if len(rr_live) else np.zeros(0, np.uint64)
    out = {k: ([], []) for k in kinds}
    for l in lr.tolist():
        match = rr_live[rk_live == limg[l]] if not lm[l] else rr_live[:0]
        for kind, (out_l, out_r) in out.items():
            if kind == "inner" or (kind == "left" and len(match)):
                out_l.extend([l + 1 + lbase] * len(match)); out_r.extend((match + 1 + rbase).tolist())
            elif kind == "left" or (kind == "anti" and not len(match)):
                out_l.append(l + 1 + lbase); out_r.append(0)
            elif kind == "semi" and len(match):
                out_l.append(l + 1 + lbase); out_r.append(int(match[0]) + 1 + rbase)
    info = (len(lr), len(rr), int(lm[lr].sum()) if len(lr) else 0, int(rm[rr].sum()) if len(rr) else 0)
    return {k: (np.array(a, np.int64), np.array(b, np.int64), info) for k, (a, b) in out.items()}


# ---------------------------------------------------------------- the columns
LEFT_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4097, 70_001)
RIGHT_COUNTS_FIXED = (0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 70_001)      # + the sort's chunk - 1, chunk, chunk + 1 (known on the device)


def unique_keys(n, lo=1000, step=3, seed=7):
    """n distinct Int64 keys lo, lo + step, .. in a random row order: the gaps between them are absent keys"""
    rng = np.random.default_rng([n, seed])
    return (lo + step * rng.permutation(n)).astype(np.int64)


def probe_keys(n, right, seed=11):
    """n Int64 keys against `right`: present keys, keys in its gaps, below its minimum and above its maximum"""
    rng = np.random.default_rng([n, seed, len(right)])
    if len(right) == 0:
        return rng.integers(-50, 50, n).astype(np.int64)
    lo, hi = int(right.min()), int(right.max())
    x = rng.integers(lo - 5, hi + 6, n).astype(np.int64)
    if n:
        pick = rng.random(n) < 0.5
        x[pick] = rng.choice(right, int(pick.sum()))
        x[:min(n, 4)] = np.array([lo - 1, hi + 1, lo, hi], np.int64)[:n]
    return x


def edge_values(dtype):
    """the values of `dtype` whose select keys are the smallest and the largest, and what lies beside them"""
    dtype = np.dtype(dtype)
    if dtype == np.bool_:
        return np.array([False, True])
    if dtype.kind in "iu":
        i = np.iinfo(dtype)
        return np.array([i.min, i.min + 1, 5, 6, i.max - 1, i.max], dtype)
    if dtype == np.float32:
        return np.concatenate([K.F32_SPECIAL_BITS.view(np.float32), np.array([1.5, -2.25, np.finfo(np.float32).max, -np.finfo(np.float32).max], np.float32)])
    return np.concatenate([K.F64_SPECIAL_BITS.view(np.float64), np.array([1.5, -2.25])])


EDGE_DTYPES = (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, np.bool_)


def edge_sides(dtype, nl=1500, nr=1300):
    """two columns of `dtype` drawn from its edge values (NaNs of several payloads, -0.0 / 0.0, the infinities, the type's minimum and maximum), the right one
    without one of them so that every kind has rows of both fates"""
    vals = edge_values(dtype)
    rng = np.random.default_rng([nl, nr, np.dtype(dtype).num])
    left = vals[rng.integers(0, len(vals), nl)]
    rvals = vals if len(vals) <= 2 else np.delete(vals, 2)
    right = rvals[rng.integers(0, len(rvals), nr)]
    if np.dtype(dtype) == np.bool_:
        right = np.zeros(nr, bool) if nr else right               # True is absent on the right
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def nullable_side(n, seed, hi=200):
    """an Int64 column with one row in five missing over garbage bytes that would match if they were read"""
    rng = np.random.default_rng([n, seed])
    x = rng.integers(0, hi, n).astype(np.int64)
    m = np.arange(n) % 5 == seed % 5
    return x, m
