"""What the String x constant match tests share (K5: `s == "c"`, `s != "c"`, startswith(s, "c"), endswith(s, "c") over a flat String column): the definition on
`bytes`, patterns whose deciding bytes sit where the kernels change behaviour, the values a subtly wrong kernel gets wrong, and column builders that
return the values with the byte total of every 1024-row tile, computed here on the host — the quantity launch_str_match chooses its form by."""
import numpy as np

from str_pair_cases import S, build  # noqa: F401  (the table pair of the String tests: bytes values, an explicit Union{String,Missing} dtype)

MODES = ("==", "!=", "startswith", "endswith")
PATTERN_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 63, 64, 65, 130)      # 8/9: one probe or two; 16/17: the tail compared from p + 16; 64/65: k_str_match
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 5 * 1024 + 77)                # every structure of these kernels is per 64 rows, per 1024-row tile or per table end
TILE = 1024
STAGE_MAX = 8144                        # launch_str_match (csrc/kernels.hpp str_match_form): a column whose largest tile holds max_tile_bytes + 48 <= 8192 is staged
DECIDING = (0, 7, 8, 15, 16)            # with the last byte: the first and last byte of each 8-byte probe and the first byte of the tail


def expect(mode, value, pat):
    """one row of `value MODE pat`: True / False, None for a missing value (as a selection that is coalesce(term, false): it selects nothing, != included)"""
    if value is None:
        return None
    if mode == "==":
        return value == pat
    if mode == "!=":
        return value != pat
    return value.startswith(pat) if mode == "startswith" else value.endswith(pat)


def term(mode, col, pat):
    """the IR of `col MODE pat`"""
    from dfdb import ir
    if mode == "==":
        return col == pat
    if mode == "!=":
        return col != pat
    return ir.startswith(col, pat) if mode == "startswith" else ir.endswith(col, pat)


def pattern(L):
    """L bytes: letters that repeat only every 26 positions, byte 0 a NUL (from 2 bytes on) and the last byte >= 0x80 — so bytes 0, 7, 8, 15, 16 and the last
    are pairwise distinct, an embedded NUL opens every pattern and a byte above 0x7f closes it"""
    p = bytearray(97 + i % 26 for i in range(L))
    if L >= 2:
        p[0] = 0
    if L >= 1:
        p[-1] |= 0x80
    return bytes(p)


def flip(pat, i):
    """pat with only byte i changed (its lowest bit)"""
    return pat[:i] + bytes([pat[i] ^ 1]) + pat[i + 1:]


def variants(pat):
    """the values a subtly wrong kernel gets wrong, each once, `pat` first"""
    L = len(pat)
    v = [pat]
    if L:
        v += [flip(pat, L - 1), flip(pat, 0)]
        v += [flip(pat, i) for i in DECIDING[1:] if i < L]
        v += [pat[:-1]]
    v += [pat + b"x", b"x" + pat, pat + pat, b"", b"zq"]
    return list(dict.fromkeys(v))


FILL = (b"", b"a", b"zq", b"\0", b"qrs", b"\xc3\xa9", b"~", b"\0\0")             # at most 3 bytes each


def tile_totals(values):
    """bytes per 1024-row tile (a missing row holds none): what K4 computes on the device"""
    sizes = np.array([0 if v is None else len(v) for v in values], np.int64)
    return [int(sizes[t:t + TILE].sum()) for t in range(0, len(values), TILE)]


def form(L, totals):
    """which form of K5 launch_str_match takes — str_match_form in csrc/kernels.hpp, restated"""
    if L > 64:
        return "long"
    return "staged" if L > 0 and 0 < max(totals) <= STAGE_MAX else "direct"


def _place_edges(rows, pat):
    """a variant at the first and last row of every tile and of the table.  A tile's last row is `pat` in every other tile and `x + pat` in the others: the
    probes of a matching last row read past the tile's end (past the arena's end in the table's last row, which is always `pat`)"""
    n = len(rows)
    for t in range(0, n, TILE):
        last = min(t + TILE, n) - 1
        odd = (t // TILE) % 2
        rows[t] = pat + b"x" if odd else pat
        rows[last] = pat if odd or last == n - 1 else b"x" + pat
    return rows


def lean(n, pat):
    """the variants once per 16 rows at a position that is no multiple of 64, fillers of at most 3 bytes otherwise: every tile holds at most 8144 bytes for
    every pattern up to 64 bytes, the staged form's condition (longer patterns go to k_str_match whatever the tiles hold)"""
    V = variants(pat)
    rows = [V[(i // 16) % len(V)] if i % 16 == 3 else FILL[(i * 5 + i // 16) % len(FILL)] for i in range(n)]
    _place_edges(rows, pat)
    totals = tile_totals(rows)
    if len(pat) <= 64:
        assert max(totals) <= STAGE_MAX, (n, len(pat), totals)
    return rows, totals


def dense(n, pat):
    """the variants back to back, and in rows 1-3 of every tile a value of 2800 bytes and more that starts with `pat` (three, because a dictionary takes no
    string above 4 KB): every tile of five rows or more exceeds 8144 bytes, so the direct form runs.  (n = 1 is the one size that cannot: a single variant
    row holds at most 2 * 130 bytes.)"""
    V = variants(pat)
    rows = [V[(i + 5) % len(V)] for i in range(n)]
    _place_edges(rows, pat)
    for t in range(0, n, TILE):
        if t + 3 < min(t + TILE, n) - 1:
            rows[t + 1:t + 4] = [pat + b"~" * (2800 + k) for k in range(3)]
    totals = tile_totals(rows)
    if n >= 5:
        assert max(totals) > STAGE_MAX, (n, len(pat), totals)
    return rows, totals


def _junk(k, i):
    return bytes(0x62 + (i + j) % 20 for j in range(k))       # never holds a pattern's first (NUL) or last (>= 0x80) byte


def edge(total, lead, pat):
    """three tiles.  Tile 0 is padded so that tile 1 starts at an arena offset of `lead` (mod 16).  Tile 1 holds exactly `total` bytes: its first row is
    `x + pat`, its last row (row 2047) is `pat`, the variants sit in its middle and the rest are fillers of the length that makes the total.  Tile 2 is
    partial and ends, as the table does, in `pat`.  With total = 8144 every tile fits the staged form; with 8145 tile 1 is the column's largest and the one byte
    flips the whole column to the direct form."""
    V = variants(pat)
    t0, _ = lean(TILE, pat)
    t0[5] = b""
    t0[5] = _junk((lead - sum(len(v) for v in t0)) % 16, 5)
    t1 = [None] * TILE
    t1[0], t1[-1] = b"x" + pat, pat
    for k, v in enumerate(V):
        t1[67 + 5 * k] = v
    free = [i for i in range(TILE) if t1[i] is None]
    rem = total - sum(len(v) for v in t1 if v is not None)
    assert rem >= 0, (total, len(pat))
    base, extra = divmod(rem, len(free))
    for k, i in enumerate(free):
        t1[i] = _junk(base + (1 if k < extra else 0), i)
    t2, _ = lean(300, pat)
    rows = t0 + t1 + t2
    totals = tile_totals(rows)
    assert totals[0] % 16 == lead and totals[1] == total and max(totals) == total, (total, lead, totals)
    assert rows[TILE] == b"x" + pat and rows[2 * TILE - 1] == pat and rows[-1] == pat
    return rows, totals


EDGE_TOTALS = (STAGE_MAX, STAGE_MAX + 1)
EDGE_LEADS = (0, 1, 15)
EDGE_LENGTHS = (8, 9, 16, 17, 64)
BUILDERS = {"lean": lean, "dense": dense}


def with_missing(rows):
    """every 7th row missing"""
    return [None if i % 7 == 6 else v for i, v in enumerate(rows)]


def selected(mode, rows, pat, keep=None):
    """0-based rows the term selects (of those `keep`, a boolean per row, lets through)"""
    return np.array([i for i, v in enumerate(rows) if expect(mode, v, pat) and (keep is None or keep[i])], np.int64)


def assert_decides(mode, rows, pat):
    """the condition on a column, from the definition alone: the expected selection holds a row and leaves a non-missing row out — so neither `all` nor `none`
    passes.  startswith / endswith with the empty pattern select every non-missing row and only that can be asked.  For == the rejected rows hold values of
    the pattern's length and of other lengths (the length shortcut alone cannot pass); the empty pattern has no other value of its length."""
    live = [v for v in rows if v is not None]
    hit = [v for v in live if expect(mode, v, pat)]
    miss = [v for v in live if not expect(mode, v, pat)]
    if len(rows) == 1:
        assert rows == [pat]                    # one row is selected or it is not: it is the pattern, which ==, startswith and endswith select and != drops
        return
    if not pat and mode in ("startswith", "endswith"):
        assert len(hit) == len(live) > 0
        return
    assert hit and miss, (mode, len(pat), len(hit), len(miss))
    if mode in ("==", "!="):
        other = miss if mode == "==" else hit
        assert any(len(v) != len(pat) for v in other)
        assert not pat or any(len(v) == len(pat) for v in other)
