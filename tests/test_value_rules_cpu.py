"""csrc/value_rules.hpp is one text for the host, the kernels and the interpreter's run-time build; its host side is pinned here without a GPU, bit for bit,
through dfdb_selftest("value_rules") (include/dfdb.h): every rule restated in numpy / struct over an edge list — ±0.0, ±inf, two NaNs with different payloads
and signs, the smallest subnormal, ±1, typemin / typemax / typemax + 1 of every integer dtype, the all-ones image — and two properties of the order image:
strictly monotonic over the sorted finite values, a NaN at the winning end."""
import ctypes as C
import struct

import numpy as np

from dfdb import ir
from dfdb import _native as N

KEY, VALUE, ORDER, MINMAX, LO, HI, WRAP, KIND, KIND_DTYPE, IDENTITY = range(10)
SIGNED, UNSIGNED, FLOAT = 0, 1, 2
INTS = {ir.I8: np.int8, ir.I16: np.int16, ir.I32: np.int32, ir.I64: np.int64, ir.U8: np.uint8, ir.U16: np.uint16, ir.U32: np.uint32, ir.U64: np.uint64}
M64 = (1 << 64) - 1


def call(fn, par, operands, is_min=False):
    out = (C.c_int64 * len(operands))(*[x - (1 << 64) if x >= (1 << 63) else x for x in operands])
    assert N.load().dfdb_selftest(b"value_rules", fn | par << 8 | int(is_min) << 16, out, len(operands)) == 0
    return [x & M64 for x in out]


def d2b(d): return struct.unpack("<Q", struct.pack("<d", d))[0]
def b2d(b): return struct.unpack("<d", struct.pack("<Q", b))[0]
def f2b(f): return struct.unpack("<I", struct.pack("<f", f))[0]


NAN_A, NAN_B = 0x7ff8000000000001, 0xfff0000000000dea        # two NaNs: quiet / signalling, either sign, different payloads
F64_FINITE = [d2b(x) for x in (-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf)]       # sorted by value (-0.0 below 0.0, as min / max order them)
F64_EDGES = F64_FINITE + [NAN_A, NAN_B, 0x7ff8000000000000, M64]                              # (all ones is a NaN)
F32_EDGES = [f2b(np.float32(x)) for x in (-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf)] + [0x00000001, 0x80000001, 0x7fc00001, 0xff800bad, 0x7fc00000, 0xffffffff]
INT_EDGES = sorted({0, 1, M64, M64 - 1} | {v & M64 for t in INTS.values() for i in [np.iinfo(t)] for v in (int(i.min), int(i.max), int(i.max) + 1, int(i.min) - 1)})


def isnan64(b): return (b & 0x7ff0000000000000) == 0x7ff0000000000000 and (b & 0x000fffffffffffff) != 0
def isnan32(b): return (b & 0x7f800000) == 0x7f800000 and (b & 0x007fffff) != 0


def test_kinds():
    for dt in INTS:
        want = SIGNED if dt in (ir.I8, ir.I16, ir.I32, ir.I64) else UNSIGNED
        assert call(KIND, dt, [0]) == [want]
    assert call(KIND, ir.BOOL, [0]) == [UNSIGNED] and call(KIND, ir.F32, [0]) == [FLOAT] and call(KIND, ir.F64, [0]) == [FLOAT]
    assert [call(KIND_DTYPE, k, [0])[0] for k in (SIGNED, UNSIGNED, FLOAT)] == [ir.I64, ir.U64, ir.F64]


def test_key_image_is_isequal():
    """integers by value (sign-extended), floats by their bits with one NaN per width; -0.0 and 0.0 stay apart"""
    assert call(KEY, ir.F64, F64_EDGES) == [0x7ff8000000000000 if isnan64(b) else b for b in F64_EDGES]
    assert call(KEY, ir.F32, F32_EDGES) == [0x7fc00000 if isnan32(b) else b for b in F32_EDGES]
    assert call(KEY, ir.F64, [d2b(-0.0)]) != call(KEY, ir.F64, [d2b(0.0)])
    for dt, t in INTS.items():
        want = [int(np.array([x & ((1 << (8 * np.dtype(t).itemsize)) - 1)], np.uint64).astype(t)[0]) & M64 for x in INT_EDGES]
        assert call(KEY, dt, INT_EDGES) == want, dt
    assert call(KEY, ir.BOOL, [0, 1, 0xff01]) == [0, 1, 1]                                   # (one byte)


def test_value_image_is_the_accumulator_operand():
    """integers widened like the key image, Float32 as the Float64 it converts to (a NaN keeps its sign and its payload, quietened: the conversion's), Float64 as it is"""
    for dt, t in INTS.items():
        assert call(VALUE, dt, INT_EDGES) == call(KEY, dt, INT_EDGES), dt
    assert call(VALUE, ir.F64, F64_EDGES) == F64_EDGES
    with np.errstate(invalid="ignore"):
        want = np.array(F32_EDGES, np.uint32).view(np.float32).astype(np.float64).view(np.uint64)      # (a NaN: its sign, its payload moved up, quietened)
    assert call(VALUE, ir.F32, F32_EDGES) == [int(w) for w in want]


def order_ref(bits, kind, is_min):
    if kind == UNSIGNED: return bits
    if kind == SIGNED: return bits ^ (1 << 63)
    if isnan64(bits): return 0 if is_min else M64
    return (~bits & M64) if bits >> 63 else bits | (1 << 63)


def test_order_image():
    for is_min in (False, True):
        for kind, edges in ((SIGNED, INT_EDGES), (UNSIGNED, INT_EDGES), (FLOAT, F64_EDGES)):
            assert call(ORDER, kind, edges, is_min) == [order_ref(b, kind, is_min) for b in edges], (kind, is_min)
        # strictly monotonic over the sorted finite values, for both float directions and both integer kinds
        f = call(ORDER, FLOAT, F64_FINITE, is_min)
        assert all(a < b for a, b in zip(f, f[1:])), (is_min, f)
        s = sorted(INT_EDGES, key=lambda b: b - (1 << 64) if b >> 63 else b)
        si = call(ORDER, SIGNED, s, is_min)
        assert all(a < b for a, b in zip(si, si[1:]))
        ui = call(ORDER, UNSIGNED, INT_EDGES, is_min)
        assert all(a < b for a, b in zip(ui, ui[1:]))
        # a NaN maps to the end that wins the reduction: below everything for a minimum, above everything for a maximum
        for nan in (NAN_A, NAN_B, M64):
            n = call(ORDER, FLOAT, [nan], is_min)[0]
            assert all(n < x for x in f) if is_min else all(n > x for x in f)
            assert n == (0 if is_min else M64)


def minmax_ref(a, b, is_min):
    """Base.min / Base.max: a NaN operand is the result (the first one), -0.0 < 0.0"""
    if isnan64(a): return a
    if isnan64(b): return b
    x, y = b2d(a), b2d(b)
    if x == y: return (a | b) if is_min else (a & b)
    return (b if y < x else a) if is_min else (b if y > x else a)


def test_minmax_f64():
    pairs = [(a, b) for a in F64_EDGES for b in F64_EDGES]
    flat = [x for p in pairs for x in p]
    for is_min in (False, True):
        got = call(MINMAX, 0, flat, is_min)
        assert got[1::2] == flat[1::2]                                                   # (the second operand of a pair stays)
        assert got[0::2] == [minmax_ref(a, b, is_min) for a, b in pairs], is_min
    z, nz = d2b(0.0), d2b(-0.0)
    assert call(MINMAX, 0, [z, nz, nz, z], True)[0::2] == [nz, nz] and call(MINMAX, 0, [z, nz, nz, z], False)[0::2] == [z, z]      # whichever came first


def test_integer_limits_and_wrap():
    for dt, t in INTS.items():
        i = np.iinfo(t)
        assert call(LO, dt, [0]) == [int(i.min) & M64] and call(HI, dt, [0]) == [int(i.max)], dt
        want = [int(np.array([x], np.uint64).astype(t)[0]) & M64 for x in INT_EDGES]            # x % T
        assert call(WRAP, dt, INT_EDGES) == want, dt
    assert call(LO, ir.F64, [0]) == [0] and call(HI, ir.F64, [0]) == [M64]                       # (anything else reads as UInt64)


def test_reduction_identities():
    inf, ninf = d2b(np.inf), d2b(-np.inf)
    assert [call(IDENTITY, FLOAT, [op])[0] for op in (N.AGG_SUM, N.AGG_MIN, N.AGG_MAX)] == [0, inf, ninf]
    assert [call(IDENTITY, SIGNED, [op])[0] for op in (N.AGG_SUM, N.AGG_MIN, N.AGG_MAX)] == [0, (1 << 63) - 1, 1 << 63]
    assert [call(IDENTITY, UNSIGNED, [op])[0] for op in (N.AGG_SUM, N.AGG_MIN, N.AGG_MAX)] == [0, M64, 0]


def test_arguments():
    out = (C.c_int64 * 3)()
    assert N.load().dfdb_selftest(b"value_rules", 99, out, 1) == N.ERR_ARGUMENT
    assert N.load().dfdb_selftest(b"value_rules", MINMAX, out, 3) == N.ERR_ARGUMENT               # pairs
