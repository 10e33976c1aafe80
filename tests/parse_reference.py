"""The yardstick of the parse tests: a Python restatement of the DFIR_CAST-over-String contract of include/dfdb_ir.h (the ASCII subset of Julia's
Base.tryparse_internal for integers, Clinger's exact fast path for Float64).  tests/test_parse_cpu.py pins it against a hand-written table.

parse_ref(dtype, s) -> (kind, value): kind is VALUE, or the name of what the engine must report for that row:
  ARGUMENT / OVERFLOW / METHOD  status DFDB_ERR_ARGUMENT, message prefix "ArgumentError:" / "OverflowError:" / "MethodError:"
  UNSUPPORTED                   status DFDB_ERR_UNSUPPORTED (a string Julia may accept and the device parser does not try)
An integer string is read left to right as Julia reads it: the first non-digit (ArgumentError) or the first digit that takes the value out of the
target's range (OverflowError) decides, whichever comes first."""
import re

I8, I16, I32, I64, U8, U16, U32, U64, F32, F64, BOOL, STRING = range(1, 13)
VALUE, ARGUMENT, OVERFLOW, METHOD, UNSUPPORTED = "value", "ArgumentError", "OverflowError", "MethodError", "Unsupported"
WS = b" \t\n\v\f\r"
RANGE = {I8: (-2**7, 2**7 - 1), I16: (-2**15, 2**15 - 1), I32: (-2**31, 2**31 - 1), I64: (-2**63, 2**63 - 1),
         U8: (0, 2**8 - 1), U16: (0, 2**16 - 1), U32: (0, 2**32 - 1), U64: (0, 2**64 - 1)}
INT_TYPES = tuple(RANGE)
_FLOAT = re.compile(rb"^([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?$")


def parse_ref(dtype, s):
    if s is None:
        return METHOD, None
    s = s.encode() if isinstance(s, str) else bytes(s)
    if any(b >= 0x80 for b in s):
        return UNSUPPORTED, None
    body = s.strip(WS)
    if not body:
        return ARGUMENT, None
    if dtype == F64:
        m = _FLOAT.match(body)
        if not m:
            return UNSUPPORTED, None
        sign, ip, fp, fp_only, ex = m.groups()
        ip, fp = (ip or b""), (fp if fp is not None else (fp_only or b""))
        e10 = int(ex or 0) - len(fp)
        if int(ip + fp) >= 2**53 or abs(e10) > 22:
            return UNSUPPORTED, None
        return VALUE, float(body)          # correctly rounded, and inside the domain one IEEE multiply or divide gives the same
    lo, hi = RANGE[dtype]
    neg, i = False, 0
    if body[:1] == b"+" or (body[:1] == b"-" and lo < 0):
        neg, i = body[:1] == b"-", 1
        if i == len(body):
            return ARGUMENT, None
        if body[i] in WS:
            return UNSUPPORTED, None
    if body[i:i + 2] in (b"0x", b"0o", b"0b"):
        return UNSUPPORTED, None
    v = 0
    for c in body[i:]:
        if not 0x30 <= c <= 0x39:
            return ARGUMENT, None
        v = v * 10 + (c - 0x30)
        if (-v < lo) if neg else (v > hi):
            return OVERFLOW, None
    return VALUE, -v if neg else v
