"""What dfdb_sort_indices_n must answer, restated in numpy on top of tests/order_stat_cases.py and tests/sort_cases.py (tests/test_sort_multi_cpu.py pins
this file on hand-written answers and on two independent statements; tests/test_gpu_sort_multi.py compares the device with it, exactly).

The order is lexicographic: cols[0] is the major key, cols[-1] the most minor.  Each key orders as sort_cases.sortperm_ref orders one column — the rows that
are not missing in it by order_stat_cases.image compared unsigned, the image complemented under that key's rev; the rows missing in it after all the others,
before them under that key's rev.  Rows equal in every key (or missing in the same keys) stay in ascending row order, whatever the revs.  The restatement is
the composition itself: the ascending selected rows re-sorted stably by each key from the most minor to the major one.

With more than one key `limit` only cuts what comes back: the device sorts every selected row, so the pairs keyed and the passes do not depend on it."""
import numpy as np

import order_stat_cases as K
import sort_cases as S


def _missing(missing, n):
    return np.zeros(n, bool) if missing is None else np.asarray(missing, bool)


def sortperm_multi_ref(cols, missings, rows=None, revs=None, limit=None) -> np.ndarray:
    """the 1-based table rows of the selected rows (`rows`: 0-based, ascending; None = all) in the order of the keys cols[0] (major) .. cols[-1]; missings[j]:
    the missing flags of cols[j] or None; revs[j]: that key descending (None: all ascending); cut to `limit` (None = all)"""
    n = len(cols[0])
    order = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    revs = [False] * len(cols) if revs is None else list(revs)
    for j in range(len(cols) - 1, -1, -1):
        v, m = np.ascontiguousarray(cols[j]), _missing(missings[j], n)
        live, miss = order[~m[order]], order[m[order]]                  # both in the order the keys behind left; the bytes under a flag are not looked at
        k = K.image(v[live])
        live = live[np.argsort(~k if revs[j] else k, kind="stable")]
        order = np.concatenate([miss, live]) if revs[j] else np.concatenate([live, miss])
    if limit is not None:
        order = order[:max(int(limit), 0)]
    return order.astype(np.int64) + 1


def pairs_multi_ref(cols, missings, rows=None) -> int:
    """info[1]: the pairs keyed, summed over the keys — each key's selected rows that are not missing in it"""
    return int(sum(len(S._split(c, m, rows)[0]) for c, m in zip(cols, missings)))


def passes_multi_ref(cols, missings, rows=None):
    """(info[2], info[3]): sort_cases.passes_ref's rule summed over the keys — per key, the bytes of narrow_key with more than one value among that key's live
    selected rows are run, its other key bytes skipped.  A key's rev complements every byte and changes neither count"""
    run = skipped = 0
    for c, m in zip(cols, missings):
        r, s = S.passes_ref(c, m, rows)
        run, skipped = run + r, skipped + s
    return run, skipped


def info_multi_ref(cols, missings, rows=None):
    n = len(cols[0])
    sel = n if rows is None else len(rows)
    return (int(sel), pairs_multi_ref(cols, missings, rows)) + passes_multi_ref(cols, missings, rows)
