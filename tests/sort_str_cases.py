"""What dfdb_sort_indices_any must answer, restated in numpy on top of tests/sort_multi_cases.py (tests/test_sort_str_cpu.py pins this file on hand-written
answers taken from Julia's rules and on an independent statement; tests/test_order_by_string_gpu.py compares the device with it, exactly).

A key is a numeric column (a numpy array, with its missing flags or None) or a String column: a list of `bytes` / None (None = missing).  isless on Strings
compares bytes as unsigned values and calls the shorter of two strings that tie the smaller; an embedded NUL is a byte like any other.  That is the
lexicographic order of the tuple (chunk_0, .., chunk_{m-1}, length): chunk_c = bytes [8c, 8c + 8) read big-endian into a uint64, zero beyond the string's end;
m = ceil(L / 8), L the largest length among the selected rows that are not missing in the key.  So a String key IS m + 1 uint64 keys of
sort_multi_cases.sortperm_multi_ref, all with the key's rev and the key's missing flags, and this file does nothing else than expand it.

info: the pairs keyed and the passes run / skipped are summed over keys AND sub-keys; a sub-key has 8 key bytes, and a byte's pass is run iff the byte takes
more than one value among the key's live selected rows."""
import numpy as np

import sort_cases as S
import sort_multi_cases as M

MAX_STRING_BYTES = 256


def is_string_key(col) -> bool:
    return isinstance(col, list)


def _rows(n, rows):
    return np.arange(n) if rows is None else np.asarray(rows, np.int64)


def sub_keys(values, rows=None):
    """(the String key's sub-keys major first — chunk_0 .. chunk_{m-1}, length — as uint64 arrays over the whole column, its missing flags)"""
    n = len(values)
    miss = np.array([v is None for v in values], bool)
    sel = _rows(n, rows)
    live = sel[~miss[sel]] if n else sel
    longest = max((len(values[int(r)]) for r in live), default=0)
    m = (longest + 7) // 8
    padded, length = np.zeros((n, 8 * m), np.uint8), np.zeros(n, np.uint64)
    for r in live:                                                      # (rows outside the selection and missing rows are never looked at)
        b = values[int(r)]
        padded[r, :len(b)] = np.frombuffer(b, np.uint8)
        length[r] = len(b)
    if m == 0:
        return [length], miss
    chunks = padded.view(">u8").astype(np.uint64)                       # [n, m]: eight bytes read big-endian, zero beyond the string's end
    return [np.ascontiguousarray(chunks[:, c]) for c in range(m)] + [length], miss


def expand(cols, missings, rows=None, revs=None):
    """(cols, missings, revs) with every String key replaced by its sub-keys"""
    revs = [False] * len(cols) if revs is None else list(revs)
    ec, em, er = [], [], []
    for c, m, r in zip(cols, missings, revs):
        if is_string_key(c):
            keys, miss = sub_keys(c, rows)
            ec += keys; em += [miss] * len(keys); er += [r] * len(keys)
        else:
            ec.append(c); em.append(m); er.append(r)
    return ec, em, er


def sortperm_any_ref(cols, missings, rows=None, revs=None, limit=None) -> np.ndarray:
    """the 1-based table rows of the selected rows in the order of the keys cols[0] (major) .. cols[-1]; as sort_multi_cases.sortperm_multi_ref"""
    ec, em, er = expand(cols, missings, rows, revs)
    return M.sortperm_multi_ref(ec, em, rows, er, limit)


def info_any_ref(cols, missings, rows=None, revs=None, limit=None):
    """(info[0..3]).  With a String key among them every selected row is sorted whatever the limit (the several-keys plan); numeric keys alone answer as
    dfdb_sort_indices_n does: one key through sort_cases (the top-k cut), several through sort_multi_cases"""
    n = len(cols[0])
    if not any(is_string_key(c) for c in cols):
        if len(cols) == 1:
            rev = bool(revs[0]) if revs is not None else False
            sel = n if rows is None else len(rows)
            return (int(sel), S.candidates_ref(cols[0], missings[0], rows, rev, limit)) + S.passes_ref(cols[0], missings[0], rows, rev, limit)
        return M.info_multi_ref(cols, missings, rows)
    ec, em, _ = expand(cols, missings, rows, revs)
    return M.info_multi_ref(ec, em, rows)
