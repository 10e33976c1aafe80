"""What dfdb_order_statistics / median / quantile must answer, restated in numpy, and the columns and selections tests/test_gpu_order_stat.py runs
(tests/test_order_stat_cpu.py pins this file on hand-written answers and checks that every column is what its name says).

The order is isless: order_image(value_image(v), value_kind(dtype), is_min = false) of csrc/value_rules.hpp compared unsigned — integers by value,
floats -Inf .. -0.0 < 0.0 .. Inf, then every NaN.  `ordered` sorts the uint64 images with np.sort and maps them back, so a NaN comes back as the
canonical quiet NaN and a Float32 as the Float64 it converts to, like the entry point's results."""
import numpy as np

QNAN_BITS = np.uint64(0x7ff8000000000000)
TOP = np.uint64(1 << 63)
ALL1 = np.uint64(0xFFFFFFFFFFFFFFFF)
ROW_COUNTS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 70_001)      # words, tiles, ctiles; 70 001: past one 65 536-row block, several workgroups, a partial last word
SHAPE_ROWS = (1025, 70_001)


def kind_of(dtype) -> str:
    dtype = np.dtype(dtype)
    return "f" if dtype.kind == "f" else ("i" if dtype.kind == "i" else "u")        # Bool is an unsigned accumulator (value_kind)


def image(values) -> np.ndarray:
    """order_image(value_image(v), value_kind(dtype), false) per element, as uint64"""
    v = np.ascontiguousarray(values)
    k = kind_of(v.dtype)
    if k == "i":
        return v.astype(np.int64).view(np.uint64) ^ TOP
    if k == "u":
        return v.astype(np.uint64)
    with np.errstate(invalid="ignore"):                                # (a signalling Float32 NaN widens to a quiet one: every NaN is one value here anyway)
        d = v.astype(np.float64)                                       # Float32 widens exactly
    bits = d.view(np.uint64)
    return np.where(np.isnan(d), ALL1, np.where(bits >> np.uint64(63) != 0, ~bits, bits | TOP))


def unimage(img, dtype) -> np.ndarray:
    """the way back: int64 / uint64 / float64 (every NaN the canonical quiet NaN)"""
    img = np.ascontiguousarray(img, np.uint64)
    k = kind_of(dtype)
    if k == "i":
        return (img ^ TOP).view(np.int64)
    if k == "u":
        return img.copy()
    bits = np.where(img == ALL1, QNAN_BITS, np.where(img >> np.uint64(63) != 0, img ^ TOP, ~img))
    return bits.astype(np.uint64).view(np.float64)


def live(values, missing=None, rows=None):
    """the selected (rows: 0-based indices, None = all), non-missing values, in table order"""
    v = np.ascontiguousarray(values)
    m = np.zeros(len(v), bool) if missing is None else np.asarray(missing, bool)
    if rows is not None:
        v, m = v[rows], m[rows]
    return v[~m]


def ordered(values, missing=None, rows=None) -> np.ndarray:
    """v[1..n]: the selected non-missing values in isless order"""
    v = np.ascontiguousarray(values)
    return unimage(np.sort(image(live(v, missing, rows))), v.dtype)


def counts(values, missing=None, rows=None):
    """(not missing, missing, NaN among the non-missing) over the selected rows"""
    v = np.ascontiguousarray(values)
    m = np.zeros(len(v), bool) if missing is None else np.asarray(missing, bool)
    if rows is not None:
        v, m = v[rows], m[rows]
    x = v[~m]
    return int(len(x)), int(m.sum()), int(np.isnan(x).sum()) if v.dtype.kind == "f" else 0


def bits_of(a) -> np.ndarray:
    """what is compared: the 64 bits of every result (floats as Float64 bits, integers widened)"""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            return a.astype(np.float64).view(np.uint64)
    if a.dtype.kind == "b":
        return a.astype(np.uint64)
    return a.astype(np.int64).view(np.uint64) if a.dtype.kind == "i" else a.astype(np.uint64)


def _f(x, dtype):
    return float(int(x)) if kind_of(dtype) != "f" else float(x)


def median_ref(values, missing=None, rows=None):
    """Statistics.median: None for missing, ValueError for ArgumentError"""
    v = np.ascontiguousarray(values)
    n, nmiss, nnan = counts(v, missing, rows)
    if nmiss:
        return None
    if n == 0:
        raise ValueError("median of an empty array is undefined")
    F = np.float32 if v.dtype == np.float32 else np.float64
    if nnan:
        return F("nan")
    s = ordered(v, missing, rows)
    mid = (1 + n) // 2
    with np.errstate(all="ignore"):
        if n % 2:
            return F(_f(s[mid - 1], v.dtype))
        return F(_f(s[mid - 1], v.dtype)) / F(2) + F(_f(s[mid], v.dtype)) / F(2)


def quantile_ref(values, p, missing=None, rows=None) -> float:
    """Statistics.quantile(v, p), default parameters, one p; ValueError for ArgumentError"""
    if not 0 <= p <= 1:
        raise ValueError("input probability out of [0,1] range")
    v = np.ascontiguousarray(values)
    n, nmiss, nnan = counts(v, missing, rows)
    if nmiss or nnan or n == 0:
        raise ValueError("quantiles are undefined for missing values, NaNs and empty data")
    s = ordered(v, missing, rows)
    if n == 1:
        return _f(s[0], v.dtype)
    aleph = n * p + (1 - p)
    j = min(max(int(np.floor(aleph)), 1), n - 1)
    g = min(max(aleph - j, 0.0), 1.0)
    a, b = np.float64(_f(s[j - 1], v.dtype)), np.float64(_f(s[j], v.dtype))
    with np.errstate(all="ignore"):
        return float(a + g * (b - a) if np.isfinite(a) and np.isfinite(b) else (1 - g) * a + g * b)


# ---------------------------------------------------------------- the columns
F64_SPECIAL_BITS = np.array([0x0000000000000000, 0x8000000000000000,            # 0.0, -0.0
                             0x7ff0000000000000, 0xfff0000000000000,            # Inf, -Inf
                             0x0000000000000001, 0x8000000000000001, 0x000fffffffffffff,      # subnormals
                             0x7ff8000000000000, 0x7ff8000000000001, 0xfff8000000000dea, 0x7ff0000000000001,      # NaN: canonical, payloads, negative, signalling
                             0x7fefffffffffffff, 0xffefffffffffffff], np.uint64)             # floatmax, -floatmax
F32_SPECIAL_BITS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x7fc00000, 0xffc00bad, 0x7f800001], np.uint32)
EQUAL_VALUE = 0x0123456789abcdef
BYTE_BASE = 0x00abcdef12345600


def _rng(name, n):
    return np.random.default_rng([n, sum(name.encode())])


def shape_column(name: str, n: int) -> np.ndarray:
    rng = _rng(name, n)
    if name == "equal":
        return np.full(n, EQUAL_VALUE, np.int64)
    if name == "low_byte":                                             # bytes 1..7 constant
        return (np.uint64(BYTE_BASE) | rng.integers(0, 256, n).astype(np.uint64)).view(np.int64)
    if name == "high_byte":                                            # bytes 0..6 constant; the sign bit varies
        return (np.uint64(BYTE_BASE >> 8) | (rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56))).view(np.int64)
    if name == "perm":
        return (rng.permutation(n) + 1).astype(np.int64)
    if name == "f64_special":
        x = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)
        k = rng.random(n) < 0.3
        x.view(np.uint64)[k] = rng.choice(F64_SPECIAL_BITS, int(k.sum()))
        x.view(np.uint64)[:min(n, len(F64_SPECIAL_BITS))] = F64_SPECIAL_BITS[:n]
        return x
    if name == "i64_extremes":
        i = np.iinfo(np.int64)
        x = rng.integers(i.min, i.max, n, dtype=np.int64, endpoint=True)
        k = rng.random(n) < 0.4
        x[k] = rng.choice(np.array([i.min, i.min + 1, -1, 0, 1, i.max - 1, i.max], np.int64), int(k.sum()))
        x[:min(n, 2)] = np.array([i.max, i.min], np.int64)[:n]
        return x
    if name == "u64_mid":
        x = (np.uint64(1 << 63) + rng.integers(-3, 4, n).astype(np.int64).view(np.uint64))
        x[rng.random(n) < 0.05] = np.uint64(0)
        x[rng.random(n) < 0.05] = ALL1
        x[:min(n, 2)] = np.array([1 << 63, (1 << 63) - 1], np.uint64)[:n]
        return x
    if name == "f32":
        x = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32)
        k = rng.random(n) < 0.2
        x.view(np.uint32)[k] = rng.choice(F32_SPECIAL_BITS, int(k.sum()))
        return x
    if name == "bool":
        return rng.random(n) < 0.3
    t = np.dtype(name)                                                 # int8 .. uint32: the whole range
    i = np.iinfo(t)
    x = rng.integers(i.min, i.max, n, dtype=t, endpoint=True)
    x[:min(n, 2)] = np.array([i.max, i.min], t)[:n]
    return x


SHAPES = ("equal", "low_byte", "high_byte", "perm", "f64_special", "i64_extremes", "u64_mid", "int8", "int16", "int32", "uint8", "uint16", "uint32", "f32", "bool")


def rowcount_column(kind: str, n: int) -> np.ndarray:
    """the columns of the row-count cases: random Float64 with a -0.0 / 0.0 pair, or random Int32"""
    rng = _rng("rows" + kind, n)
    if kind == "f64":
        x = rng.standard_normal(n)
        x[rng.random(n) < 0.1] = 0.0
        x[rng.random(n) < 0.1] = -0.0
        return x
    return rng.integers(-2**31, 2**31, n).astype(np.int32)


# ---------------------------------------------------------------- selections over N_SEL rows: the column `x`, a uniform 0..99 column `u`, a column `t` = row ÷ 3000
N_SEL = 70_001


def selection_table():
    rng = _rng("selections", N_SEL)
    x = rng.standard_normal(N_SEL) * 1000.0
    u = rng.integers(0, 100, N_SEL).astype(np.int64)
    t = (np.arange(N_SEL) // 3000).astype(np.int64)
    return x, u, t


def selections(u, t):
    """name -> (the selector of a view, the 0-based rows it keeps).  Selectors: ("range", start, step), ("indices", 1-based list), ("pred", column, op, constant)"""
    n = len(u)
    idx = np.sort(_rng("index list", n).choice(n, 777, replace=False))
    return {
        "none": (None, np.arange(n)),
        "range": (("range", 1, 7), np.arange(0, n, 7)),
        "indices": (("indices", (idx + 1).tolist()), idx),
        "pred10": (("pred", "u", "<", 10), np.flatnonzero(u < 10)),
        "nothing": (("pred", "u", "<", 0), np.zeros(0, np.int64)),
        "empty_tiles": (("pred", "t", "==", 5), np.flatnonzero(t == 5)),          # rows 15 000 .. 17 999: every other 1024-row tile is empty
    }


# ---------------------------------------------------------------- a nullable column whose missing rows hold garbage that would win rank 1 and rank n
def nullable_column(n: int, all_missing: bool = False):
    rng = _rng("nullable", n)
    x = rng.standard_normal(n)
    m = np.ones(n, bool) if all_missing else (np.arange(n) % 7 == 6)
    g = np.flatnonzero(m)
    x[g[0::3]] = -np.inf
    x.view(np.uint64)[g[1::3]] = np.uint64(0x7ff8000000000bad)         # NaN: last in the order, and it would count as NaN
    x[g[2::3]] = np.inf
    return x, m
