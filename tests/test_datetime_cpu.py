"""datetime19(s) without a device: the IR bytes of the front end, the header's enumerator, and the tests' own yardstick (tests/datetime_reference.py)
against known answers, the calendar of the standard library and numpy.  (Typing and refusals need a table: tests/test_gpu_datetime.py has them.)"""
import datetime
import os
import re

import numpy as np
import pytest

from datetime_reference import ARGUMENT, BOUNDS, RATA_DIE_MS, UNSUPPORTED, VALUE, datetime_ref, totaldays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_datetime19_emits_the_cast_with_its_target():
    import dfdb
    from dfdb import ir
    assert ir.datetime19(ir.col(2)).to_ir() == bytes.fromhex("01 02000000 50") + bytes([ir.CAST_DATETIME])
    assert ir.datetime19(ir.col(2)).to_ir() == bytes.fromhex("01 02000000 50 44")
    assert "datetime19" in dfdb.__all__
    assert dfdb.datetime19(ir.col(0)).to_ir() == bytes.fromhex("01 00000000 50 44")
    assert (ir.datetime19(ir.col(1)) >= np.datetime64("2019-10-02", "ms")).to_ir()[:7] == bytes.fromhex("01 01000000 50 44")


def test_the_headers_enumerator_is_the_front_ends():
    from dfdb import ir
    txt = open(os.path.join(ROOT, "include", "dfdb_ir.h")).read()
    m = re.search(r"DFDB_CAST_DATETIME\s*=\s*0x([0-9a-fA-F]+)\s*\|\s*DFDB_I64", txt)
    assert m and (int(m.group(1), 16) | ir.I64) == ir.CAST_DATETIME
    assert ir.CAST_DATETIME & ~(ir.DTYPE_MASK | ir.NULLABLE)            # outside the dtypes and not the nullable flag: no dtype is mistaken for it
    assert ir.CAST_DATETIME & ir.DTYPE_MASK == ir.I64 and ir.RATA_DIE_MS == RATA_DIE_MS


@pytest.mark.parametrize("s,ms", [("2019-10-01 00:00:11 UTC", 63705571211000), ("1970-01-01 00:00:00", 62135683200000), ("0000-01-01 00:00:00", -31536000000)])
def test_known_answers(s, ms):
    assert datetime_ref(s) == (VALUE, ms)
    assert datetime_ref(s.encode()) == (VALUE, ms)


def test_totaldays_is_the_proleptic_gregorian_ordinal():
    years = [1, 4, 100, 400, 1582, 1600, 1899, 1900, 1901, 1999, 2000, 2001, 2019, 2020, 2021, 2022, 2023, 2024, 2100, 9999]
    for y in years:
        day = datetime.date(y, 1, 1)
        while day.year == y:
            assert totaldays(day.year, day.month, day.day) == day.toordinal(), day
            if day == datetime.date.max:
                break
            day += datetime.timedelta(days=1)
    assert totaldays(0, 1, 1) == -365 and totaldays(0, 12, 31) == 0 and totaldays(0, 2, 29) == -365 + 31 + 28      # year 0000 is a leap year


def test_values_agree_with_numpy_on_a_random_sample():
    rng = np.random.default_rng(19)
    for _ in range(3000):
        y, mo, h, mi, s = int(rng.integers(1, 10000)), int(rng.integers(1, 13)), int(rng.integers(0, 24)), int(rng.integers(0, 60)), int(rng.integers(0, 60))
        d = int(rng.integers(1, 29))
        txt = f"{y:04d}-{mo:02d}-{d:02d} {h:02d}:{mi:02d}:{s:02d}"
        want = int(np.datetime64(txt.replace(" ", "T"), "ms").astype(np.int64)) + RATA_DIE_MS
        assert datetime_ref(txt + " UTC") == (VALUE, want), txt


ROWS = [
    (None, BOUNDS),                                                      # rule 1: string(missing) is 7 bytes
    ("2019-10-01 00:00:0", BOUNDS),                                      # 18 ASCII bytes
    ("", BOUNDS),
    ("2019-10-01 00:00é", UNSUPPORTED),                             # 18 bytes, one >= 0x80: rule 1 needs ALL bytes < 0x80, so this is rule 2
    ("2019-13-01 00:00:00", ARGUMENT),
    ("2019-00-10 00:00:00", ARGUMENT),
    ("2019-02-29 00:00:00", ARGUMENT), ("2020-02-29 00:00:00", VALUE),
    ("1900-02-29 00:00:00", ARGUMENT), ("2000-02-29 00:00:00", VALUE),
    ("2019-04-31 00:00:00", ARGUMENT), ("2019-04-00 00:00:00", ARGUMENT),
    ("2019-10-01 24:61:00", UNSUPPORTED),                                # hour 24 with a bad minute: rule 5, not rule 4
    ("2019-10-01 24:00:00", UNSUPPORTED),
    ("2019-13-01 24:00:00", ARGUMENT),                                   # the month comes first
    ("2019-10-01 25:00:00", ARGUMENT),
    ("2019-10-01 23:60:00", ARGUMENT), ("2019-10-01 23:59:60", ARGUMENT),
    (" 019-10-01 00:00:00", UNSUPPORTED),                                # parse(Int64, " 019") is a value in Julia: not decided here
    ("+019-10-01 00:00:00", UNSUPPORTED), ("2019-1a-01 00:00:00", UNSUPPORTED),
    ("2019é10-01 00:00:00", UNSUPPORTED),                           # a non-ASCII separator at byte 4 (two bytes wide: every later index moves)
    (b"2019\xff10-01 00:00:00", UNSUPPORTED),
    ("2019-10-01 00:00:00é", VALUE), (b"2019-10-01 00:00:00\xff\xfe", VALUE),      # from byte 19 on nothing is read
    ("2019-10-01T00:00:00.123", VALUE), ("2019x10y01z00w00v00", VALUE),                  # the separators are ignored
]


@pytest.mark.parametrize("s,kind", ROWS)
def test_one_row_per_rule_and_per_ordering(s, kind):
    k, v = datetime_ref(s)
    assert k == kind, (s, k)
    assert (v is not None) == (kind == VALUE)


def test_ignored_bytes_do_not_change_the_value():
    want = datetime_ref("2019-10-01 00:00:00")
    for s in ("2019-10-01 00:00:00 UTC", "2019-10-01T00:00:00", "2019-10-01T00:00:00.123"):
        assert datetime_ref(s) == want
    assert want == (VALUE, int(np.datetime64("2019-10-01", "ms").astype(np.int64)) + RATA_DIE_MS)
