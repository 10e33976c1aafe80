"""What dfdb_sort_indices must answer, restated in numpy on top of tests/order_stat_cases.py (tests/test_sort_cpu.py pins this file on hand-written
Julia answers; tests/test_gpu_sort.py compares the device with it, exactly).

The order is the one of order_stat_cases.image — isless: integers by value, floats -Inf .. -0.0 < 0.0 .. Inf, then every NaN — compared unsigned, the image
complemented for `rev`.  np.argsort(kind="stable") keeps ties in ascending row order in both directions, like Julia's sortperm (rev reverses the ordering,
not the ties).  Missing rows come after the others (before them under rev) in row order; the bytes under a missing flag are never looked at.

Pass counts: the device sorts on the SELECT KEY of csrc/select_key.hpp, the same order restated in the column's own width (`narrow_key`), 8 bits per pass,
and skips the pass of every key byte that has one value in all the pairs it sorts.  The missing rows are not pairs — they are compacted into a list of their
own —, so the implementation spends NO pass on a missing flag: passes_ref adds nothing for a nullable column."""
import numpy as np

import order_stat_cases as K


def _split(values, missing, rows):
    """(0-based selected rows that are not missing, 0-based selected rows that are missing), both ascending"""
    v = np.ascontiguousarray(values)
    m = np.zeros(len(v), bool) if missing is None else np.asarray(missing, bool)
    rows = np.arange(len(v)) if rows is None else np.asarray(rows, np.int64)
    return rows[~m[rows]], rows[m[rows]]


def sortperm_ref(values, missing=None, rows=None, rev=False, limit=None) -> np.ndarray:
    """the 1-based table rows of the selected rows (`rows`: 0-based, ascending; None = all) in sortperm order, cut to `limit` (None = all)"""
    v = np.ascontiguousarray(values)
    lv, ms = _split(v, missing, rows)
    k = K.image(v[lv])
    o = lv[np.argsort(~k if rev else k, kind="stable")]
    res = np.concatenate([ms, o]) if rev else np.concatenate([o, ms])
    if limit is not None:
        res = res[:max(int(limit), 0)]
    return res.astype(np.int64) + 1


def live_in_limit(nlive, nmiss, rev, limit):
    """L: how many of the first `limit` results are not missing"""
    if limit is None or limit < 0:
        return nlive
    return max(0, min(limit - nmiss, nlive)) if rev else min(limit, nlive)


def _candidates(values, missing, rows, rev, limit):
    """the 0-based rows the device sorts: the live rows whose key does not exceed the key of rank L in the sort direction (all of them when L = nlive, none
    when L = 0)"""
    v = np.ascontiguousarray(values)
    lv, ms = _split(v, missing, rows)
    L = live_in_limit(len(lv), len(ms), rev, limit)
    if L == 0:
        return lv[:0]
    if L == len(lv):
        return lv
    k = K.image(v[lv])
    k = ~k if rev else k
    return lv[k <= np.sort(k)[L - 1]]


def candidates_ref(values, missing=None, rows=None, rev=False, limit=None) -> int:
    """info[1]: the pairs sorted"""
    return int(len(_candidates(values, missing, rows, rev, limit)))


def narrow_key(values) -> np.ndarray:
    """select_key<DT, false> of csrc/select_key.hpp per element, as uint64: the order of K.image in the 8 * W bits of a W-byte value"""
    v = np.ascontiguousarray(values)
    w = v.dtype.itemsize
    if w == 8:
        return K.image(v)
    if v.dtype.kind == "f":                                            # Float32
        b = v.view(np.uint32)
        k = np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(0x80000000))
        return np.where(np.isnan(v), np.uint32(0xFFFFFFFF), k).astype(np.uint64)
    u = v.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[w]).astype(np.uint64)
    return u ^ np.uint64(1 << (8 * w - 1)) if v.dtype.kind == "i" else u


def key_bytes(dtype) -> int:
    return np.dtype(dtype).itemsize


def passes_ref(values, missing=None, rows=None, rev=False, limit=None):
    """(info[2], info[3]): the digit passes run — the key bytes with more than one distinct value among the pairs sorted — and skipped (the other key bytes).
    Nothing is added for a nullable column: the missing rows never enter the sort."""
    v = np.ascontiguousarray(values)
    k = narrow_key(v[_candidates(v, missing, rows, rev, limit)])
    nb = key_bytes(v.dtype)
    run = sum(1 for b in range(nb) if len(np.unique((k >> np.uint64(8 * b)) & np.uint64(255))) > 1)
    return run, nb - run
