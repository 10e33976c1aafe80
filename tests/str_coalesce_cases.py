"""What the String coalesce tests share: the rule of `coalesce(a, b)` over String columns restated on Python lists of `bytes | None`, the flat form the
engine and the oracle hand back (Int32 sizes, -1 for missing, and one byte arena), and the case table: row contents, missing patterns, defaults.

The oracle's own coalesce is numeric only, so this restatement is the yardstick; it is applied to what the oracle (or the input lists) say the source
columns hold.  tests/test_str_coalesce_cpu.py pins it by a literal known-answer table."""
import numpy as np


def coalesce_ref(a, b):
    """Julia's coalesce.(a, b): row i is a[i] unless it is missing, else b[i]; b is a list (a column) or one `bytes` (a constant).  A row missing on
    both sides stays missing."""
    if isinstance(b, (bytes, bytearray)):
        b = [bytes(b)] * len(a)
    assert len(a) == len(b)
    return [y if x is None else x for x, y in zip(a, b)]


def flat(values):
    """list of bytes | None -> (sizes int32 with -1 for missing, arena uint8, total bytes)"""
    sizes = np.array([-1 if v is None else len(v) for v in values], np.int32)
    raw = b"".join(v for v in values if v is not None)
    return sizes, np.frombuffer(raw, np.uint8).copy(), len(raw)


def unflat(sizes, data):
    """(sizes, arena) -> list of bytes | None"""
    out, o, raw = [], 0, np.asarray(data, np.uint8).tobytes()
    for s in np.asarray(sizes).tolist():
        if s < 0:
            out.append(None)
        else:
            out.append(raw[o:o + s]); o += s
    assert o == len(raw), (o, len(raw))
    return out


# ---------------------------------------------------------------- the case table
N = 3 * 1024 + 37                                   # tile boundaries, a ragged last tile, 64-row group tails
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 300)
EMPTY_TILE = 1                                      # every row of this 1024-row tile is the empty string


def row_strings(n=N, salt=0):
    """lengths 0, 1, 7, 8, 9, 15, 16, 17 (and 300 every 41st row), bytes >= 0x80 and an embedded NUL in every row long enough, one tile of empty strings"""
    out = []
    for i in range(n):
        ln = 300 if i % 41 == 40 else LENGTHS[(i * 7 + i // 64 + salt) % 8]
        s = bytearray((33 + (i * 31 + k * 7 + salt) % 90) for k in range(ln))
        if ln >= 7:
            s[1], s[3], s[5] = 0xC3, 0x00, 0xFF
        out.append(bytes(s))
    if salt == 0:
        for i in range(EMPTY_TILE * 1024, min(n, (EMPTY_TILE + 1) * 1024)):
            out[i] = b""
    return out


def missing_patterns(n=N):
    """name -> boolean mask of the rows of `a` that are missing"""
    k = np.arange(n)
    return {
        "none": np.zeros(n, bool),
        "all": np.ones(n, bool),
        "every7th": k % 7 == 0,
        "first": k == 0,
        "last": k == n - 1,
        "tile2": (k >= 2 * 1024) & (k < 3 * 1024),
        "run-over-boundary": (k >= 1024 - 70) & (k < 1024 + 70),
    }


def with_missing(values, mask):
    return [None if m else v for v, m in zip(values, mask)]


CONSTANTS = [b"", b"?", b"missing", b"8 bytes!", b"nine byte", b"seventeen bytes !", b"a default of forty bytes, not one less!!", "fehlt éÿ".encode() + b"\xfe\x80"]
assert [len(c) for c in CONSTANTS[:7]] == [0, 1, 7, 8, 9, 17, 40]


def default_columns(n=N):
    """(a plain String column, a nullable String column): the nullable one is missing on every third row, so on some of the rows where `a` is missing under
    each pattern above that has more than a few missing rows"""
    plain = row_strings(n, salt=3)
    nullable = with_missing(row_strings(n, salt=5), np.arange(n) % 3 == 0)
    return plain, nullable
