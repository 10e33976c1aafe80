"""The definition and the shared inputs of the String gather at given rows (dfdb_gather_rows_any, csrc/k_str_rows.hip), for test_str_gather_rows_cpu.py and
test_gpu_str_gather_rows.py.

The definition: take_ref(values, rows) is [values[r - 1] for r in rows] — `rows` are 1-based table rows, in any order, with repeats — flattened to what
dfdb_materialize writes for a String column: int32 sizes with -1 for None, and the bytes of the rows concatenated in that order.

The columns: string lengths cycle through 0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17 and 300 BYTES (every branch of copy_string: whole 8-byte moves, the 4 / 2 / 1
byte tail stores, nothing at all), two rows in three carry a multi-byte UTF-8 character; one nullable column has every 5th row missing, another a whole
1024-row tile.  Nothing is larger than 70 001 rows."""
import numpy as np

LENGTHS = (0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 300)
COLUMN_ROWS = (1, 1023, 1024, 1025, 2049, 70_001)
COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4097)
TILE = 1024


def string_of(i):
    """row i's string: LENGTHS[i % 12] bytes of UTF-8 that depend on i"""
    nbytes = LENGTHS[i % len(LENGTHS)]
    head = ""
    if i % 3 == 0 and nbytes >= 3:
        head = "€"                                  # 3 bytes
    elif i % 3 == 1 and nbytes >= 2:
        head = "é"                                  # 2 bytes
    k = nbytes - len(head.encode())
    s = head + "".join(chr(97 + (i * 7 + j * 3) % 26) for j in range(k))
    assert len(s.encode()) == nbytes
    return s


def missing_tile(nrows):
    """the 1024-row tile the `tile` column misses whole: the second one when there is one"""
    return 1 if nrows > TILE else 0


def columns(nrows):
    """name -> list of str / None: `plain` (no row missing), `fifth` (every 5th row missing), `tile` (one whole tile missing)"""
    plain = [string_of(i) for i in range(nrows)]
    fifth = [None if i % 5 == 4 else s for i, s in enumerate(plain)]
    mt = missing_tile(nrows)
    tile = [None if i // TILE == mt else s for i, s in enumerate(plain)]
    return {"plain": plain, "fifth": fifth, "tile": tile}


NULLABLE = ("fifth", "tile")


def row_lists(nrows):
    """name -> int64 array of 1-based rows of a column of nrows rows"""
    rng = np.random.default_rng(nrows)
    last_tile = (nrows - 1) // TILE
    one_tile = missing_tile(nrows)
    out = {
        "empty": [],
        "one": [nrows // 2 + 1],
        "first_last": [1, nrows],
        "tile_edges": [1, min(TILE, nrows), last_tile * TILE + 1, nrows],
        "ascending": np.arange(1, nrows + 1),
        "reversed": np.arange(nrows, 0, -1),
        "permutation": rng.permutation(nrows) + 1,
        "repeat1500": np.full(1500, (nrows * 2) // 3 + 1),
        "one_tile": np.arange(one_tile * TILE + 1, min((one_tile + 1) * TILE, nrows) + 1),
    }
    for n in COUNTS:
        out[f"n{n}"] = rng.integers(1, nrows + 1, n)
    return {k: np.asarray(v, np.int64) for k, v in out.items()}


def flatten(picked):
    """a list of str / bytes / None -> (int32 sizes, -1 for None; uint8 bytes)"""
    enc = [None if v is None else (v.encode() if isinstance(v, str) else bytes(v)) for v in picked]
    sizes = np.array([-1 if e is None else len(e) for e in enc], np.int32)
    data = np.frombuffer(b"".join(e for e in enc if e), np.uint8).copy()
    return sizes, data


def take_ref(values, rows):
    return flatten([values[int(r) - 1] for r in rows])
