"""datetime19(s), the tutorial's fixed-position timestamp conversion, restated in pure Python from the rule table of include/dfdb_ir.h (DFIR_CAST with the
target DFDB_CAST_DATETIME).  It takes nothing from the engine: the GPU tests compare the engine with it bit for bit (tests/test_datetime_cpu.py pins it)."""
VALUE, BOUNDS, ARGUMENT, UNSUPPORTED = "value", "bounds", "argument", "unsupported"

SHIFT = (306, 337, 0, 31, 61, 92, 122, 153, 184, 214, 245, 275)
FIELDS = ((0, 4), (5, 7), (8, 10), (11, 13), (14, 16), (17, 19))       # byte ranges of year, month, day, hour, minute, second
RATA_DIE_MS = 62135683200000                                            # DateTime(1970, 1, 1).instant in milliseconds


def totaldays(y, m, d):
    """Dates.totaldays: days since 0000-12-31, floored divisions (Python's // floors)"""
    z = y - 1 if m < 3 else y
    return d + SHIFT[m - 1] + 365 * z + z // 4 - z // 100 + z // 400 - 306


def isleap(y):
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def daysinmonth(y, m):
    return (31, 29 if isleap(y) else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)[m - 1]


def datetime_ref(s):
    """s: str, bytes or None (a missing row) -> (kind, value); value is the Int64 millisecond instant for VALUE, else None"""
    if s is None:
        return BOUNDS, None                                             # rule 1: string(missing) is 7 bytes long
    b = s.encode("utf8") if isinstance(s, str) else bytes(s)
    n = len(b)
    head = b[:min(n, 19)]
    if n < 19 and all(c < 0x80 for c in head):
        return BOUNDS, None                                             # rule 1
    if any(c >= 0x80 for c in head):
        return UNSUPPORTED, None                                        # rule 2
    vals = []
    for lo, hi in FIELDS:
        f = b[lo:hi]
        if not all(0x30 <= c <= 0x39 for c in f):
            return UNSUPPORTED, None                                    # rule 3
        vals.append(int(f))
    y, m, d, h, mi, sec = vals
    if not 1 <= m <= 12:
        return ARGUMENT, None                                           # rule 4 ...
    if not 1 <= d <= daysinmonth(y, m):
        return ARGUMENT, None
    if h > 24:
        return ARGUMENT, None
    if h == 24:
        return UNSUPPORTED, None                                        # rule 5: also with a bad minute or second
    if mi >= 60 or sec >= 60:
        return ARGUMENT, None                                           # ... rule 4
    return VALUE, 1000 * (sec + 60 * mi + 3600 * h + 86400 * totaldays(y, m, d))
