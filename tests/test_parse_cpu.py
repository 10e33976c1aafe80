"""parse(T, s) without a device: the IR bytes of the front end and the tests' own yardstick (tests/parse_reference.py) against a hand-written table.
(Typing and refusals need a table, and a table needs a context: tests/test_gpu_parse.py has them.)"""
import math
import struct

import pytest

import parse_reference as R
from parse_reference import ARGUMENT, METHOD, OVERFLOW, UNSUPPORTED, VALUE, parse_ref


def test_parse_emits_cast_over_the_column():
    from dfdb import ir
    assert ir.parse(ir.I64, ir.col(0)).to_ir() == bytes.fromhex("01 00000000 50 04")
    assert ir.parse(ir.F64, ir.col(3)).to_ir() == bytes.fromhex("01 03000000 50 0a")
    # cast() of a String-typed Expr is the same bytes: DFIR_CAST over a String operand MEANS parse
    assert ir.cast(ir.col(0), ir.I64).to_ir() == ir.parse(ir.I64, ir.col(0)).to_ir()
    # inside a larger expression
    assert (ir.parse(ir.U8, ir.col(1)) % 7).to_ir() == bytes.fromhex("01 01000000 50 05 02 04 0700000000000000 15")


def test_parse_is_exported_beside_sizeof():
    import dfdb
    from dfdb import ir
    assert "parse" in dfdb.__all__ and "sizeof" in dfdb.__all__
    assert dfdb.parse(ir.I32, ir.col(2)).to_ir() == bytes.fromhex("01 02000000 50 03")


# (dtype, string, outcome, value)
TABLE = [
    (R.I64, "0", VALUE, 0), (R.I64, "12", VALUE, 12), (R.I64, "+12", VALUE, 12), (R.I64, "-12", VALUE, -12), (R.I64, "-0", VALUE, 0),
    (R.I64, "007", VALUE, 7), (R.I64, "  42\t\n", VALUE, 42), (R.I64, "\v\f\r9 ", VALUE, 9),
    (R.I64, "9223372036854775807", VALUE, 2**63 - 1), (R.I64, "-9223372036854775808", VALUE, -2**63),
    (R.I64, "9223372036854775808", OVERFLOW, None), (R.I64, "-9223372036854775809", OVERFLOW, None),
    (R.I64, "00000000000000000000000000001", VALUE, 1),
    (R.I8, "127", VALUE, 127), (R.I8, "-128", VALUE, -128), (R.I8, "128", OVERFLOW, None), (R.I8, "-129", OVERFLOW, None),
    (R.I8, "1000a", OVERFLOW, None), (R.I8, "12a", ARGUMENT, None),
    (R.U8, "255", VALUE, 255), (R.U8, "256", OVERFLOW, None), (R.U8, "-1", ARGUMENT, None), (R.U8, "+1", VALUE, 1), (R.U8, "-0", ARGUMENT, None),
    (R.U16, "65535", VALUE, 65535), (R.U32, "4294967296", OVERFLOW, None), (R.I16, "-32768", VALUE, -32768), (R.I32, "2147483648", OVERFLOW, None),
    (R.U64, "18446744073709551615", VALUE, 2**64 - 1), (R.U64, "18446744073709551616", OVERFLOW, None),
    (R.I64, "", ARGUMENT, None), (R.I64, "   ", ARGUMENT, None), (R.I64, "+", ARGUMENT, None), (R.I64, "-", ARGUMENT, None), (R.I64, "1 2", ARGUMENT, None),
    (R.I64, "12x", ARGUMENT, None), (R.I64, "x12", ARGUMENT, None), (R.I64, "1.5", ARGUMENT, None), (R.I64, "1_000", ARGUMENT, None),
    (R.I64, None, METHOD, None), (R.F64, None, METHOD, None),
    (R.I64, "- 5", UNSUPPORTED, None), (R.I64, "+\t5", UNSUPPORTED, None), (R.I64, "0x10", UNSUPPORTED, None), (R.I64, "-0b1", UNSUPPORTED, None),
    (R.I64, "0o7", UNSUPPORTED, None), (R.I64, "12\u00a0", UNSUPPORTED, None), (R.I64, "\u20031", UNSUPPORTED, None), (R.I64, "\uff11\uff12", UNSUPPORTED, None),
    (R.F64, "35.79", VALUE, 35.79), (R.F64, ".5", VALUE, 0.5), (R.F64, "5.", VALUE, 5.0), (R.F64, "-0.0", VALUE, -0.0), (R.F64, "1e22", VALUE, 1e22),
    (R.F64, " 1.25E-3 ", VALUE, 0.00125), (R.F64, "+9007199254740991", VALUE, 9007199254740991.0), (R.F64, "0.1", VALUE, 0.1),
    (R.F64, "123456789012345e-37", UNSUPPORTED, None), (R.F64, "1234567.5e-3", VALUE, 1234.5675),
    (R.F64, "9007199254740992", UNSUPPORTED, None), (R.F64, "0.1234567890123456789", UNSUPPORTED, None), (R.F64, "1e23", UNSUPPORTED, None),
    (R.F64, "1e-23", UNSUPPORTED, None), (R.F64, "Inf", UNSUPPORTED, None), (R.F64, "NaN", UNSUPPORTED, None), (R.F64, "0x1p3", UNSUPPORTED, None),
    (R.F64, "1f3", UNSUPPORTED, None), (R.F64, "1_0.5", UNSUPPORTED, None), (R.F64, ".", UNSUPPORTED, None), (R.F64, "1e", UNSUPPORTED, None),
    (R.F64, "- 1.5", UNSUPPORTED, None), (R.F64, "", ARGUMENT, None), (R.F64, " \t", ARGUMENT, None),
]


@pytest.mark.parametrize("dtype,s,kind,value", TABLE)
def test_reference_against_the_table(dtype, s, kind, value):
    got_kind, got = parse_ref(dtype, s)
    assert got_kind == kind, (dtype, s, got_kind, got)
    if kind == VALUE:
        if dtype == R.F64:
            assert struct.pack("<d", got) == struct.pack("<d", value) and math.copysign(1.0, got) == math.copysign(1.0, value)
        else:
            assert got == value and isinstance(got, int)


def test_reference_equals_python_on_valid_input():
    """what the issue fixes as the yardstick's own check: int(s) for valid integers, float(s) inside the exact domain"""
    for dtype, s, kind, _ in TABLE:
        if kind != VALUE:
            continue
        got = parse_ref(dtype, s)[1]
        if dtype == R.F64:
            assert struct.pack("<d", got) == struct.pack("<d", float(s))
        else:
            assert got == int(s)
