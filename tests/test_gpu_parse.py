"""parse(T, s) on the device: DFIR_CAST over a String column (include/dfdb_ir.h).  The yardstick is tests/parse_reference.py, the Python restatement of the
contract (tests/test_parse_cpu.py pins it); every comparison is bit-exact, every error is checked by status, message prefix and reported row."""
import re

import numpy as np
import pytest

import parse_reference as R
from parse_reference import ARGUMENT, METHOD, OVERFLOW, UNSUPPORTED, VALUE, parse_ref

pytestmark = pytest.mark.gpu

BS = 65536
NP = {R.I8: np.int8, R.I16: np.int16, R.I32: np.int32, R.I64: np.int64, R.U8: np.uint8, R.U16: np.uint16, R.U32: np.uint32, R.U64: np.uint64,
      R.F64: np.float64}
PADS = ["", " ", "\t", "\n", "\v", "\f", "\r", "  \t "]


@pytest.fixture(params=[0, 2], ids=["jit0", "jit2"])
def jit(ctx, request):
    """every case under the ahead-of-time interpreter and under its run-time compiled form"""
    ctx.set_option("jit", request.param)
    ctx.set_option("jit_min_rows", 0)
    yield request.param
    ctx.set_option("jit", 1)
    ctx.set_option("jit_min_rows", 1 << 22)


@pytest.fixture(params=[1, 0], ids=["kernel", "interp"])
def path(ctx, request):
    """a projected `parse.(T, s)` through the conversion kernel k_str_parse, and through the interpreter's H_PARSE (csrc/KNOBS.md: parse_kernel)"""
    ctx.set_option("parse_kernel", request.param)
    yield request.param
    ctx.set_option("parse_kernel", 1)


def launches(ctx, fn):
    """(k_str_parse launches, interpreter or compiled-interpreter projection launches) while fn runs"""
    names = ("str_parse", "interp_project", "jit_project")
    ctx.profile(True)
    before = [ctx.profile_get(k)[0] for k in names]
    try:
        fn()
    finally:
        after = [ctx.profile_get(k)[0] for k in names]
        ctx.profile(False)
    return after[0] - before[0], after[1] - before[1] + after[2] - before[2]


def table_of(dfdb, strs, nullable=False, extra=None):
    from dfdb import ir
    t = dfdb.DFTable.new(block_size=BS)
    t.add_column("s", list(strs), dtype=ir.STRING | (ir.NULLABLE if nullable else 0))
    for k, v in (extra or {}).items():
        t.add_column(k, v)
    return t


def project(dfdb, t, fn, sel=None):
    v = dfdb.DFView(t)
    if sel is not None:
        v = v[sel, dfdb.ALL]
    return dfdb.materialize(v[dfdb.ALL, {"r": ("s", fn)}])["r"].to_numpy()


def expected(dtype, strs):
    out = []
    for s in strs:
        k, v = parse_ref(dtype, s)
        assert k == VALUE, (s, k)
        out.append(v)
    return np.array(out, dtype=NP[dtype])


def same_bits(got, want):
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.nonzero(got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1))[0]
    assert len(bad) == 0, (int(bad[0]), got[bad[0]], want[bad[0]])


def int_strings(dtype, rng, per_len=60):
    """valid strings of every digit count up to the type's widest, the type's limits, leading zeros, `+`, whitespace padding"""
    lo, hi = R.RANGE[dtype]
    out = [str(lo), str(hi), "0", "-0" if lo < 0 else "+0", "+" + str(hi), "000" + str(hi), " " + str(lo) + "\t", "0" * 40 + "7"]
    for nd in range(1, len(str(hi)) + 1):
        top = min(hi, 10**nd - 1)
        for _ in range(per_len):
            v = int(rng.integers(10**(nd - 1) if nd > 1 else 0, top, endpoint=True, dtype=np.uint64))
            neg = lo < 0 and rng.random() < 0.5
            if neg and v > -lo:
                v = -lo
            s = ("-" if neg else ("+" if rng.random() < 0.2 else "")) + "0" * int(rng.integers(0, 3)) + str(v)
            out.append(PADS[int(rng.integers(0, len(PADS)))] + s + PADS[int(rng.integers(0, len(PADS)))])
    return out


def float_strings(rng, n):
    """in-domain only: significand (point removed) < 2^53 and |power of ten| <= 22"""
    out = ["35.79", ".5", "5.", "-0.0", "0.0", "+1e22", "1E-22", "9007199254740991", "0.1", "123456.789e3", " 2.50\t", "-.25e+2"]
    while len(out) < n:
        nd = int(rng.integers(1, 16))
        digits = "".join(str(int(d)) for d in rng.integers(0, 10, nd))
        point = int(rng.integers(0, nd + 1))
        form = int(rng.integers(0, 4))
        if form == 0:                                   # fixed-point price
            s = (digits[:point] or "0") + "." + digits[point:]
            e10 = -(nd - point)
        elif form == 1:                                 # integer
            s, e10 = digits, 0
        else:                                           # e form
            ex = int(rng.integers(-22 + (nd - point), 23))
            s = digits[:point] + "." + digits[point:] + ("e" if form == 2 else "E") + (("+" if rng.random() < 0.3 else "") if ex >= 0 else "") + str(ex)
            e10 = ex - (nd - point)
        if abs(e10) > 22:
            continue
        out.append(("-" if rng.random() < 0.3 else "") + s)
    return out


# ---------------------------------------------------------------- typing
def test_result_type_is_the_target_and_never_nullable(dfdb_mod, ctx):
    from dfdb import ir
    t = table_of(dfdb_mod, ["1", "2"], extra={"k": np.arange(2, dtype=np.int64)})
    tn = table_of(dfdb_mod, ["1", None])
    for dt in R.INT_TYPES + (R.F64,):
        assert t.expr_dtype(ir.parse(dt, ir.col(0))) == dt
        assert tn.expr_dtype(ir.parse(dt, ir.col(0))) == dt          # parse(T, ::Missing) is a MethodError, not missing
    assert t.expr_dtype(ir.parse(ir.I64, ir.col(0)) > 5) == ir.BOOL
    assert tn.expr_dtype(ir.parse(ir.I32, ir.col(0)) % 7) == ir.I64
    for bad in (ir.BOOL, ir.F32, ir.STRING, ir.I64 | ir.NULLABLE):
        with pytest.raises(NotImplementedError, match="unsupported conversion"):
            t.expr_dtype(ir.cast(ir.col(0), bad))
    assert t.expr_dtype(ir.cast(ir.col(1), ir.I8)) == ir.I8          # a numeric operand: still Julia's T(x)


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("dtype", R.INT_TYPES)
def test_every_integer_target(dfdb_mod, ctx, jit, path, dtype):
    from dfdb import ir
    strs = int_strings(dtype, np.random.default_rng(dtype))
    t = table_of(dfdb_mod, strs)
    want = expected(dtype, strs)
    same_bits(project(dfdb_mod, t, lambda s: ir.parse(dtype, s)), want)
    same_bits(project(dfdb_mod, t, lambda s: ir.cast(s, dtype)), want)


def test_float64_in_domain_is_correctly_rounded(dfdb_mod, ctx, jit, path):
    from dfdb import ir
    strs = float_strings(np.random.default_rng(11), 20_000)
    kinds = [parse_ref(R.F64, s)[0] for s in strs]
    assert all(k == VALUE for k in kinds), [s for s, k in zip(strs, kinds) if k != VALUE][:5]      # the generator stays inside the domain: nothing is refused
    t = table_of(dfdb_mod, strs)
    got = project(dfdb_mod, t, lambda s: ir.parse(ir.F64, s))
    same_bits(got, np.array([float(s) for s in strs], np.float64))
    assert np.signbit(got[strs.index("-0.0")]) and got[strs.index("-0.0")] == 0.0
    same_bits(project(dfdb_mod, t, lambda s: ir.parse(ir.F64, s) * 1), got * 1)


@pytest.mark.parametrize("bad", ["0.1234567890123456789", "1e23", "Inf", "NaN", "1f3", "0x1p3", "1_0.5", "12345678901234567890"])
@pytest.mark.parametrize("row", [777, BS + 4321])
def test_float64_out_of_domain_is_refused_with_its_row(dfdb_mod, ctx, jit, path, bad, row):
    from dfdb import ir
    strs = ["1.5"] * (2 * BS + 100)
    strs[row] = bad
    strs[row + 50] = "1e400"
    t = table_of(dfdb_mod, strs)
    with pytest.raises(NotImplementedError, match=rf"\(row {row}\)"):
        project(dfdb_mod, t, lambda s: ir.parse(ir.F64, s))


# ---------------------------------------------------------------- where parse runs
@pytest.fixture(scope="module")
def digits(dfdb_mod, ctx):
    """the tutorial's shape: 19-digit decimal strings in a Union{String,Missing} column without missing rows, several blocks"""
    rng = np.random.default_rng(5)
    n = 3 * BS + 12_345
    vals = rng.integers(10**18, 2**63 - 1, n, dtype=np.int64)
    strs = [str(int(v)) for v in vals]
    t = table_of(dfdb_mod, strs, nullable=True, extra={"k": np.arange(n, dtype=np.int64)})
    return t, vals


def test_materialize_selection_predicate_and_larger_expressions(dfdb_mod, ctx, jit, path, digits):
    from dfdb import ir
    t, vals = digits
    n = len(vals)
    same_bits(project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s)), vals)
    keep = np.arange(n) % 10 == 3                                                       # a selection, then materialize: compacted output
    same_bits(project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s), sel=ir.col(1) % 10 == 3), vals[keep])
    same_bits(project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s) % 7), np.fmod(vals, 7))
    same_bits(project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s) + 0), vals)
    same_bits(project(dfdb_mod, t, lambda s: ir.parse(ir.U64, s) + ir.parse(ir.I64, s)), vals.astype(np.uint64) * 2)
    c = int(np.median(vals))
    v = dfdb_mod.DFView(t)[ir.parse(ir.I64, ir.col(0)) > c, dfdb_mod.ALL]
    assert np.array_equal(v._query().indices(), np.nonzero(vals > c)[0] + 1)
    v2 = dfdb_mod.DFView(t)[(ir.parse(ir.I64, ir.col(0)) > c) & (ir.col(1) % 3 == 0), dfdb_mod.ALL]
    assert np.array_equal(v2._query().indices(), np.nonzero((vals > c) & (np.arange(n) % 3 == 0))[0] + 1)
    same_bits(dfdb_mod.materialize(v2[dfdb_mod.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s) % 7)}])["r"].to_numpy(),
              np.fmod(vals, 7)[(vals > c) & (np.arange(n) % 3 == 0)])


def test_add_column_from_a_parsed_column(dfdb_mod, ctx, jit, path, digits):
    from dfdb import ir
    t, vals = digits
    t2 = table_of(dfdb_mod, ["x"] * len(vals))
    t2.add_column_from("id", dfdb_mod.DFView(t)[dfdb_mod.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s))}])
    assert t2.columns_meta()[1].dtype == ir.I64
    same_bits(dfdb_mod.materialize(dfdb_mod.DFView(t2)[dfdb_mod.ALL, ["id"]])["id"].to_numpy(), vals)


def test_the_compiled_kernel_is_the_one_that_runs_under_jit2(dfdb_mod, ctx, digits):
    from dfdb import ir
    t, vals = digits
    ctx.set_option("jit", 2)
    ctx.set_option("jit_min_rows", 0)
    try:
        ctx.profile(True)
        same_bits(project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s) % 9), np.fmod(vals, 9))
        nj, ni = ctx.profile_get("jit_project")[0], ctx.profile_get("interp_project")[0]
        ctx.profile(False)
    finally:
        ctx.set_option("jit", 1)
        ctx.set_option("jit_min_rows", 1 << 22)
    assert nj >= 1 and ni == 0, (nj, ni)


# ---------------------------------------------------------------- errors
ERRORS = [("12a", ARGUMENT), ("", ARGUMENT), (" \t ", ARGUMENT), ("-", ARGUMENT), ("1 2", ARGUMENT), ("99999999999999999999", OVERFLOW),
          ("-9223372036854775809", OVERFLOW), (None, METHOD), ("0x10", UNSUPPORTED), ("- 5", UNSUPPORTED), ("12\u00a0", UNSUPPORTED), ("12\xff".encode("latin1"), UNSUPPORTED)]
EXC = {ARGUMENT: ValueError, OVERFLOW: ValueError, METHOD: ValueError, UNSUPPORTED: NotImplementedError}
PREFIX = {ARGUMENT: "ArgumentError: ", OVERFLOW: "OverflowError: ", METHOD: "MethodError: no method matching parse", UNSUPPORTED: "parse: "}


def raises(kind, row):
    return pytest.raises(EXC[kind], match="^" + re.escape(PREFIX[kind]) + rf".*\(row {row}\)$")


@pytest.mark.parametrize("bad,kind", ERRORS)
@pytest.mark.parametrize("row", [1500, 2 * BS + 99])
def test_each_error_kind_with_its_row(dfdb_mod, ctx, jit, path, bad, kind, row):
    from dfdb import ir
    assert parse_ref(R.I64, bad)[0] == kind
    strs = ["123"] * (3 * BS)
    strs[row] = bad
    t = table_of(dfdb_mod, strs, nullable=True)
    with raises(kind, row):                                      # a computed projection column
        project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s))
    with raises(kind, row):                                      # inside a larger expression
        project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s) % 7)
    with raises(kind, row):                                      # a predicate
        dfdb_mod.DFView(t)[ir.parse(ir.I64, ir.col(0)) > 5, dfdb_mod.ALL]._query().indices()
    t2 = table_of(dfdb_mod, ["x"] * len(strs))
    with raises(kind, row):                                      # add_column!
        t2.add_column_from("id", dfdb_mod.DFView(t)[dfdb_mod.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s))}])
    assert len(t2.columns_meta()) == 1


def test_unsigned_target_refuses_the_minus_sign_and_small_targets_overflow(dfdb_mod, ctx, jit, path):
    from dfdb import ir
    strs = ["7"] * 5000
    strs[4000], strs[4500] = "-1", "300"
    t = table_of(dfdb_mod, strs)
    with raises(ARGUMENT, 4000):
        project(dfdb_mod, t, lambda s: ir.parse(ir.U8, s))
    with raises(OVERFLOW, 4500):
        project(dfdb_mod, t, lambda s: ir.parse(ir.I16, s) + ir.parse(ir.I8, s))
    same_bits(project(dfdb_mod, t, lambda s: ir.parse(ir.I16, s)), expected(R.I16, strs))


@pytest.mark.parametrize("first,second", [(OVERFLOW, UNSUPPORTED), (UNSUPPORTED, ARGUMENT), (METHOD, OVERFLOW), (ARGUMENT, METHOD)])
def test_the_smaller_row_decides_between_two_kinds(dfdb_mod, ctx, jit, path, first, second):
    from dfdb import ir
    sample = {ARGUMENT: "1x", OVERFLOW: "9" * 30, METHOD: None, UNSUPPORTED: "0b1"}
    strs = ["5"] * (2 * BS)
    strs[BS - 1], strs[BS] = sample[first], sample[second]                       # neighbours in different blocks
    t = table_of(dfdb_mod, strs, nullable=True)
    with raises(first, BS - 1):
        project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s))
    with raises(first, BS - 1):
        dfdb_mod.DFView(t)[ir.parse(ir.I64, ir.col(0)) == 5, dfdb_mod.ALL]._query().indices()
    # beside the kinds that were there before: 1 ÷ 0 on an earlier row wins, on a later row loses
    t.add_column("z", np.where(np.arange(len(strs)) == 10, 0, 1).astype(np.int64))
    with pytest.raises(ZeroDivisionError):
        dfdb_mod.DFView(t)[(ir.parse(ir.I64, ir.col(0)) == 5) & (ir.div(1, ir.col(1)) == 1), dfdb_mod.ALL]._query().indices()
    t.add_column("z2", np.where(np.arange(len(strs)) == BS + 10, 0, 1).astype(np.int64))
    with raises(first, BS - 1):
        dfdb_mod.DFView(t)[(ir.parse(ir.I64, ir.col(0)) == 5) & (ir.div(1, ir.col(2)) == 1), dfdb_mod.ALL]._query().indices()


def test_a_missing_row_raises_only_where_it_is_selected(dfdb_mod, ctx, jit, path):
    from dfdb import ir
    n, row = 2 * BS + 7, BS + 3
    strs = [str(i) for i in range(n)]
    strs[row] = None
    t = table_of(dfdb_mod, strs, extra={"k": np.arange(n, dtype=np.int64)})
    want = np.delete(np.arange(n, dtype=np.int64), row)
    same_bits(project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s), sel=ir.col(1) != row), want)
    with raises(METHOD, row):
        project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s), sel=ir.col(1) >= row)
    with raises(METHOD, row):
        project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s))
    # two predicate stages in a row are ONE fused `&` in the reference (selection.jl:44-47), not short-circuit: the second one is evaluated on every row
    # that reached the pair, as a DivideError there is — the engine's existing rule for raising predicates
    v = dfdb_mod.DFView(t)[ir.col(1) != row, dfdb_mod.ALL][ir.parse(ir.I64, ir.col(0)) % 2 == 1, dfdb_mod.ALL]
    with raises(METHOD, row):
        v._query().indices()
    # behind a range stage that ends before the row's block nothing is evaluated there
    v = dfdb_mod.DFView(t)[dfdb_mod.jr(1, BS - 5), dfdb_mod.ALL][ir.parse(ir.I64, ir.col(0)) % 2 == 1, dfdb_mod.ALL]
    assert np.array_equal(v._query().indices(), np.nonzero(np.arange(BS - 5) % 2 == 1)[0] + 1)


# ---------------------------------------------------------------- the two paths
def messy_strings(rng, n):
    """what a real import holds: mostly plain digits of every length, and everything the fast path must hand over — padding, signs, 20 digits, other
    characters, empty and missing rows, values outside the target"""
    out = []
    odd = ["", " ", "+", "-", "12a", "0x10", "- 5", "1 2", "1e3", "99999999999999999999", "18446744073709551615", "-9223372036854775808", "9223372036854775808",
           " 42\t", "+7", "-0", "0000000000000000000000012", None, "12\u00a0", "255", "256", "-129", "65536", "4294967296", "2147483648"]
    for _ in range(n):
        r = rng.random()
        if r < 0.08:
            out.append(odd[int(rng.integers(0, len(odd)))])
        else:
            nd = int(rng.integers(1, 21))
            s = "".join(str(int(d)) for d in rng.integers(0, 10, nd))
            out.append(("-" if r < 0.3 else "") + s)
    return out


@pytest.mark.parametrize("dtype", R.INT_TYPES + (R.F64,))
def test_kernel_and_interpreter_agree_row_by_row(dfdb_mod, ctx, jit, dtype):
    """value, error kind and error row of a messy column, through k_str_parse and through H_PARSE, both against the reference.  All the rows that have a
    value at once (an index-list selection: the SELECTED form of the kernel); and, for a sample of the rows that have none, the selection that starts at
    that row, of which it is the first error"""
    from dfdb import ir
    rng = np.random.default_rng(100 + dtype)
    strs = messy_strings(rng, 6000)
    t = table_of(dfdb_mod, strs, nullable=True, extra={"k": np.arange(len(strs), dtype=np.int64)})
    ref = [parse_ref(dtype, s) for s in strs]
    bad_rows = [i for i, (k, _) in enumerate(ref) if k != VALUE]
    good = np.array([k == VALUE for k, _ in ref])
    assert len(bad_rows) > 100 and good.sum() > 300
    want_good = np.array([v for k, v in ref if k == VALUE], dtype=NP[dtype])
    sel = (np.nonzero(good)[0] + 1).tolist()
    results = {}
    for knob in (1, 0):
        ctx.set_option("parse_kernel", knob)
        try:
            v = dfdb_mod.DFView(t)[sel, dfdb_mod.ALL][dfdb_mod.ALL, {"r": ("s", lambda s: ir.parse(dtype, s))}]
            nk, ni = launches(ctx, lambda: results.__setitem__(knob, dfdb_mod.materialize(v)["r"].to_numpy()))
            assert (nk >= 1 and ni == 0) if knob else (nk == 0 and ni >= 1), (knob, nk, ni)      # the path the knob names is the one that ran
            same_bits(results[knob], want_good)
            for row in bad_rows[:: max(1, len(bad_rows) // 25)]:
                with raises(ref[row][0], row):
                    project(dfdb_mod, t, lambda s: ir.parse(dtype, s), sel=ir.col(1) >= row)
        finally:
            ctx.set_option("parse_kernel", 1)
    same_bits(results[1], results[0])


def test_long_strings_take_the_direct_path(dfdb_mod, ctx, jit, path):
    """a tile whose bytes do not fit the LDS stage is parsed straight from the arena; its neighbours are staged"""
    from dfdb import ir
    strs = [str(i) for i in range(5000)]
    for i in range(1024, 2048):
        strs[i] = " " * 40 + str(i) + " " * 3                      # 1024 rows x 47 bytes: above the stage
    t = table_of(dfdb_mod, strs)
    same_bits(project(dfdb_mod, t, lambda s: ir.parse(ir.I32, s)), np.arange(5000, dtype=np.int32))
    strs[1500] = " " * 40 + "x"
    with raises(ARGUMENT, 1500):
        project(dfdb_mod, table_of(dfdb_mod, strs), lambda s: ir.parse(ir.I32, s))


PARSE_STAGE = 19968          # the bytes a wave stages for parse (csrc/k_parse.hip: ParseConv::kStage)


def stage_edge_rows(rng, lead, tile1_bytes):
    """2048 rows, the two tiles of one workgroup: Int64 digit strings of up to 19 bytes, the second row of each tile widened with whitespace to the tile's
    byte total.  Tile 0 holds the most bytes that are staged and leave tile 1 `lead` bytes above a 16-byte boundary; tile 1 holds tile1_bytes"""
    strs = []
    for total in (PARSE_STAGE - 16 - (16 - lead) % 16, tile1_bytes):
        rows = []
        for _ in range(1024):
            nd = 19 if rng.random() < 0.8 else int(rng.integers(1, 19))
            v = int(rng.integers(10**18, 2**63 - 1, dtype=np.int64)) if nd == 19 else int(rng.integers(10**(nd - 1) if nd > 1 else 0, 10**nd))
            rows.append(("-" if nd < 19 and rng.random() < 0.3 else "") + str(v))
        pad = total - sum(len(r) for r in rows)
        assert pad > 0, pad
        rows[1] = " " * (pad // 2) + rows[1] + "\t" * (pad - pad // 2)
        strs += rows
    return strs


@pytest.mark.parametrize("lead", [0, 15])
def test_the_largest_staged_tile_and_the_smallest_direct_tile(dfdb_mod, ctx, lead):
    """a tile `lead` bytes above a 16-byte boundary is staged exactly when its bytes + lead + 16 <= PARSE_STAGE: the tile that fills the stage to its last
    byte, and the same tile one byte longer, which is parsed from the arena.  Both tiles belong to one workgroup, whose two stages are neighbours in LDS"""
    from dfdb import ir
    staged = stage_edge_rows(np.random.default_rng(1900 + lead), lead, PARSE_STAGE - 16 - lead)
    direct = list(staged)
    direct[1025] += " "
    for strs, over in ((staged, 0), (direct, 1)):
        size = [len(s) for s in strs]
        assert len(size) == 2048 and max(len(s.strip()) for s in strs) <= 19
        assert sum(size[:1024]) % 16 == lead and sum(size[:1024]) + 16 <= PARSE_STAGE          # tile 0, at lead 0, is staged
        assert sum(size[1024:]) + lead + 16 == PARSE_STAGE + over
    want = expected(R.I64, staged)
    same_bits(expected(R.I64, direct), want)
    ctx.set_option("parse_kernel", 1)
    got = []
    for strs in (staged, direct):
        t = table_of(dfdb_mod, strs)
        nk, ni = launches(ctx, lambda: got.append(project(dfdb_mod, t, lambda s: ir.parse(ir.I64, s))))
        assert nk >= 1 and ni == 0, (nk, ni)
        same_bits(got[-1], want)
    same_bits(got[0], got[1])


@pytest.mark.parametrize("bad,kind", [("12a", ARGUMENT), ("9" * 25, OVERFLOW), ("0x10", UNSUPPORTED), ("1\u2003", UNSUPPORTED), (None, METHOD)])
def test_a_parsed_divisor_reports_the_parse_outcome_not_a_divide_error(dfdb_mod, ctx, jit, bad, kind):
    """a row without a value goes on as 0, so `x ÷ parse(T, s)` meets a division by zero of its own on the same row: the parse outcome is the one reported
    (the leaf is evaluated first; for an UNSUPPORTED string Julia returns a value, and the caller must get status 7 to fall back)"""
    from dfdb import ir
    n, row = 2 * BS, BS + 77
    strs = ["3"] * n
    strs[row] = bad
    t = table_of(dfdb_mod, strs, nullable=True, extra={"k": np.arange(n, dtype=np.int64)})
    for f in (lambda s, k: ir.div(k, ir.parse(ir.I64, s)), lambda s, k: k % ir.parse(ir.I64, s), lambda s, k: ir.mod(k, ir.parse(ir.I64, s)),
              lambda s, k: ir.rem(k, ir.parse(ir.I32, s))):
        with raises(kind, row):                                  # a projection
            dfdb_mod.materialize(dfdb_mod.DFView(t)[dfdb_mod.ALL, {"r": (("s", "k"), f)}])
        with raises(kind, row):                                  # a predicate
            dfdb_mod.DFView(t)[f(ir.col(0), ir.col(1)) == 0, dfdb_mod.ALL]._query().indices()
    # a genuine zero divisor still raises DivideError, and an earlier one still wins
    strs[row] = "0"
    t0 = table_of(dfdb_mod, strs, nullable=True, extra={"k": np.arange(n, dtype=np.int64)})
    with pytest.raises(ZeroDivisionError):
        dfdb_mod.materialize(dfdb_mod.DFView(t0)[dfdb_mod.ALL, {"r": (("s", "k"), lambda s, k: ir.div(k, ir.parse(ir.I64, s)))}])
    strs[row], strs[row - 5] = bad, "0"
    t1 = table_of(dfdb_mod, strs, nullable=True, extra={"k": np.arange(n, dtype=np.int64)})
    with pytest.raises(ZeroDivisionError):
        dfdb_mod.DFView(t1)[ir.div(ir.col(1), ir.parse(ir.I64, ir.col(0))) == 0, dfdb_mod.ALL]._query().indices()


def test_parse_of_a_lazy_column(dfdb_mod, ctx, jit, path, digits):
    """dfdb.parse(T, t.s): the DFColumn form of the front end"""
    from dfdb import ir
    t, vals = digits
    col = dfdb_mod.parse(ir.I64, dfdb_mod.DFView(t).s)
    assert isinstance(col, dfdb_mod.DFColumn) and col.eltype == ir.I64
    same_bits(np.asarray(dfdb_mod.materialize(col)), vals)
    t2 = table_of(dfdb_mod, ["x"] * len(vals))
    t2.add_column_from("id", col)
    same_bits(dfdb_mod.materialize(dfdb_mod.DFView(t2)[dfdb_mod.ALL, ["id"]])["id"].to_numpy(), vals)


@pytest.mark.parametrize("bad,kind", [("12a", ARGUMENT), ("9" * 25, OVERFLOW), ("0x10", UNSUPPORTED), (None, METHOD)])
def test_errors_out_of_core_carry_the_table_row(dfdb_mod, ctx, jit, path, tmp_path, bad, kind):
    """a bad row in a later chunk of a table that is answered block-streamed from its files: the reported row is the table's, not the chunk's"""
    from dfdb import ir
    n, row = 5 * BS + 11, 3 * BS + 500
    strs = [str(i) for i in range(n)]
    strs[row] = bad
    strs[row + BS] = "zz"
    t = table_of(dfdb_mod, strs, nullable=True, extra={"k": np.arange(n, dtype=np.int64)})
    p = str(tmp_path / "tb")
    t.save(p)
    t3 = dfdb_mod.open_table(p, load=False)
    try:
        t3.ctx.set_option("ooc_chunk_blocks", 2)
        with raises(kind, row):
            dfdb_mod.materialize(dfdb_mod.DFView(t3)[dfdb_mod.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s))}])
        with raises(kind, row):
            dfdb_mod.DFView(t3)[ir.parse(ir.I64, ir.col(0)) % 2 == 0, dfdb_mod.ALL]._query().count()
        assert not t3.resident(0)
        want = np.arange(row, dtype=np.int64)
        same_bits(dfdb_mod.materialize(dfdb_mod.DFView(t3)[ir.col(1) < row, dfdb_mod.ALL][dfdb_mod.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s))}])["r"].to_numpy(), want)
    finally:
        t3.close()


# ---------------------------------------------------------------- the tutorial's workflow
def test_import_convert_save_and_reopen(dfdb_mod, oracle, ctx, jit, path, digits, tmp_path):
    """route A: add_column!(t, :id, parse.(Int64, t.s)), save, the oracle's reader reads the new column back;
    route B: the saved table reopened with nothing resident answers materialize(parse.(Int64, s)) out of core.  Both equal the reference."""
    from dfdb import ir
    t0, vals = digits
    strs = [str(int(v)) for v in vals]
    want = expected(R.I64, strs)
    same_bits(want, vals)
    t = table_of(dfdb_mod, strs, nullable=True)
    assert t.columns_meta()[0].dtype == ir.STRING | ir.NULLABLE
    t.add_column_from("id", dfdb_mod.DFView(t)[dfdb_mod.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s))}])
    assert t.columns_meta()[1].dtype == ir.I64
    path = str(tmp_path / "tb")
    assert t.save(path)["rows"] == len(vals)
    route_a = oracle.Table.open(path).view().materialize()[1]
    same_bits(np.asarray(route_a), want)
    t3 = dfdb_mod.open_table(path, load=False)
    try:
        t3.ctx.set_option("ooc_chunk_blocks", 2)
        v = dfdb_mod.DFView(t3)[dfdb_mod.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s))}]
        route_b = dfdb_mod.materialize(v)["r"].to_numpy()
        assert not t3.resident(0)
        same_bits(route_b, want)
        same_bits(route_b, np.asarray(route_a))
        keep = vals % 10 == 3
        vs = dfdb_mod.DFView(t3)[ir.col(1) % 10 == 3, dfdb_mod.ALL][dfdb_mod.ALL, {"r": ("s", lambda s: ir.parse(ir.I64, s) % 7)}]
        same_bits(dfdb_mod.materialize(vs)["r"].to_numpy(), np.fmod(vals, 7)[keep])
    finally:
        t3.close()
