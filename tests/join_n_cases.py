"""What dfdb_query_join_n / dfdb_query_join_fetch must answer, restated in Python, and the columns tests/test_join_n_gpu.py runs (tests/test_join_n_cpu.py pins
this file on hand-written answers, on tests/join_cases.py for one key and on pandas.merge).

A side is a list of COMPONENTS, the major key first.  A component is (values, missing): a numpy array with missing flags (None: none), or — a String key — a
list of bytes / str / None (None: the row is missing; the second entry is ignored).  A row's key is the Python tuple of its components: a fixed-width component
is its order image (tests/order_stat_cases.py `image`: every NaN one value, -0.0 and 0.0 two, integers by value), a String component is its bytes — so "a" and
"a\\0" differ and the empty string is a key.  A row with ANY component missing matches nothing.  The result is two parallel lists of 1-based table rows, ordered
by left row and within one left row by right row; right row 0 = no match."""
import numpy as np

import order_stat_cases as K
from join_cases import KINDS, KIND_CODE  # noqa: F401  (the tests take them from here)


def is_string(values):
    return isinstance(values, (list, tuple))


def as_bytes(v):
    return None if v is None else (v.encode() if isinstance(v, str) else bytes(v))


def component_keys(values, missing):
    """per row: the component's key (an int image or bytes), or None when it is missing"""
    if is_string(values):
        return [as_bytes(v) for v in values]
    arr = np.ascontiguousarray(values)
    img = K.image(arr).tolist() if len(arr) else []
    if missing is None:
        return img
    return [None if m else k for k, m in zip(img, np.asarray(missing, bool).tolist())]


def side_keys(comps):
    """per row: the tuple of its components, or None when any of them is missing"""
    per = [component_keys(v, m) for v, m in comps]
    return [None if any(x is None for x in row) else row for row in zip(*per)]


def join_n_ref_all(lcomps, lrows, rcomps, rrows, lbase=0, rbase=0, kinds=KINDS):
    """kind -> (left_rows, right_rows, info[0:4]).  lrows / rrows: the 0-based selected rows, ascending (None: all).  Every selected left row, ascending, is
    compared with every selected right row, ascending, by their tuples (the comparison runs through a dict from tuple to the right rows that hold it)"""
    lkeys, rkeys = side_keys(lcomps), side_keys(rcomps)
    lr = list(range(len(lkeys))) if lrows is None else [int(x) for x in lrows]
    rr = list(range(len(rkeys))) if rrows is None else [int(x) for x in rrows]
    where = {}
    for r in rr:
        if rkeys[r] is not None:
            where.setdefault(rkeys[r], []).append(r)
    out = {k: ([], []) for k in kinds}
    for l in lr:
        match = where.get(lkeys[l], []) if lkeys[l] is not None else []
        for kind, (out_l, out_r) in out.items():
            if kind == "inner" or (kind == "left" and match):
                out_l.extend([l + 1 + lbase] * len(match)); out_r.extend(r + 1 + rbase for r in match)
            elif kind == "left" or (kind == "anti" and not match):
                out_l.append(l + 1 + lbase); out_r.append(0)
            elif kind == "semi" and match:
                out_l.append(l + 1 + lbase); out_r.append(match[0] + 1 + rbase)
    info = (len(lr), len(rr), sum(lkeys[l] is None for l in lr), sum(rkeys[r] is None for r in rr))
    return {k: (np.array(a, np.int64), np.array(b, np.int64), info) for k, (a, b) in out.items()}


def join_n_ref(lcomps, lrows, rcomps, rrows, kind, lbase=0, rbase=0):
    return join_n_ref_all(lcomps, lrows, rcomps, rrows, lbase, rbase, (kind,))[kind]


def chunks_of(strings):
    """m: the 8-byte chunks of the longest live string (0: none is live, or all are empty)"""
    return max([(len(as_bytes(s)) + 7) // 8 for s in strings if s is not None], default=0)


# ---------------------------------------------------------------- the columns
LEFT_COUNTS_2 = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4097)
RIGHT_COUNTS_2 = (0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025)
STRING_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 256)


def pair_sides(nl, nr, seed=5, hi0=7, hi1=9):
    """two Int64 key columns per side drawn from small ranges: tuples that match in both components, in the first only, in the second only, in neither"""
    rng = np.random.default_rng([nl, nr, seed])
    left = [rng.integers(0, hi0, nl).astype(np.int64), rng.integers(0, hi1, nl).astype(np.int64)]
    right = [rng.integers(1, hi0 + 1, nr).astype(np.int64), rng.integers(1, hi1 + 1, nr).astype(np.int64)]
    return left, right


def string_pool():
    """byte strings of every length of STRING_LENGTHS: shared prefixes that differ only in the last chunk or only in length, trailing and embedded NULs,
    multi-byte UTF-8"""
    base = bytes((i * 37 + 11) % 251 + 1 for i in range(256))            # no NUL inside
    pool = [base[:n] for n in STRING_LENGTHS]
    pool += [base[:16] + b"\x00", base[:15] + b"\x01", base[:8] + b"\x00" * 8, base[:8] + b"\x00" * 7, base[:255] + b"\xff", base[:255] + b"\xfe"]
    pool += [b"a", b"a\x00", b"a\x00\x00", b"\x00", b"\x00\x00", b"a\x00b", b"a\x00c", b"ab"]
    pool += ["żółw".encode(), "żółć".encode(), "日本語のキー".encode(), "日本語のキ".encode(), "é".encode(), "e".encode()]
    return pool


def string_sides(nl, nr, seed=3, drop=2):
    """a String column per side drawn from string_pool(); the right side lacks every `drop`-th string of the pool, so that every kind has rows of both fates"""
    pool = string_pool()
    rng = np.random.default_rng([nl, nr, seed])
    rpool = [s for i, s in enumerate(pool) if i % drop != 1] if drop else pool
    left = [pool[i] for i in rng.integers(0, len(pool), nl)]
    right = [rpool[i] for i in rng.integers(0, len(rpool), nr)]
    return left, right


def with_missing(values, which):
    """a String column with the rows of `which` (bool per row) missing"""
    return [None if m else v for v, m in zip(values, np.asarray(which, bool).tolist())]
