"""The 2-byte coarse copy kept beside the 4-byte scan image (csrc/scan_coarse.hpp, k_image.hip k_scan_coarse_build, k_scan.hip k_scan_cmp_coarse, scan_route.hpp, scan_image.cpp): a
lone `col OP const` scan of an Int64 / UInt64 column that has an image reads 2 bytes per row and settles the rows its coarse value leaves undecided from the
4-byte image.  Every answer must be the flat column's bit for bit, and numpy's, as a fresh mask and behind a range stage; and the profile notes must say WHICH
form ran — the coarse kernel, the exact 2-byte scan (span below 65536), or the 4-byte scan (constant outside [min, max], or a dense bucket) — so that a
fallback cannot pass for the coarse path.  The expected form is worked out here from the column and the constant by the issue's rule, not read from the engine."""
import operator

import numpy as np
import pytest

from helpers import Pair

pytestmark = pytest.mark.gpu

OPS = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}
I32_MIN, I32_MAX, U32_MAX = -(1 << 31), (1 << 31) - 1, (1 << 32) - 1
MIN_ROWS_DEFAULT = 1 << 24
# the edges of a lane's 8 rows, a wave load's 512, a tile, a four-tile trip; two trips and a bit; many trips
SIZES = [1, 7, 8, 9, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 5, 65536 + 17]
KEYS = ("scan_cmp", "scan_image", "scan_image.build", "scan_image.coarse_build", "scan_image.coarse", "scan_image.coarse_exact", "scan_image.coarse_dense")
FORMS = {  # the profile of one scan by the form that must have run: exactly one launch under scan_image, the note of that form alone
    "coarse": {"scan_image.coarse": 1, "scan_image.coarse_exact": 0, "scan_image.coarse_dense": 0},
    "exact": {"scan_image.coarse": 0, "scan_image.coarse_exact": 1, "scan_image.coarse_dense": 0},
    "dense": {"scan_image.coarse": 0, "scan_image.coarse_exact": 0, "scan_image.coarse_dense": 1},
    "image": {"scan_image.coarse": 0, "scan_image.coarse_exact": 0, "scan_image.coarse_dense": 0},
}


@pytest.fixture()
def coarse_ctx(ctx):
    """the session's context with the image (and its coarse copy) built at the first eligible scan of any size; the library's defaults afterwards"""
    ctx.set_option("scan_image", 2)
    ctx.set_option("scan_image_min_rows", 1)
    ctx.set_option("scan_coarse", 1)
    try:
        yield ctx
    finally:
        ctx.profile(False)
        ctx.set_option("scan_image", 1)
        ctx.set_option("scan_image_min_rows", MIN_ROWS_DEFAULT)
        ctx.set_option("scan_coarse", 1)


def image_bytes(ctx):
    return ctx.profile_get("scan_image_bytes")[0]


def expected_form(x, c, scan_coarse):
    """the issue's rule, from the column's values: which form a scan of `x OP c` takes when the column has an image and a coarse copy"""
    mn, mx = int(x.min()), int(x.max())
    if c < mn or c > mx:
        return "image"
    shift = max(0, (mx - mn).bit_length() - 16)
    if shift == 0:
        return "exact"
    if scan_coarse == 2:
        return "coarse"
    coarse = (x.astype(np.int64) - mn) >> shift               # (every value here fits 33 bits)
    in_bin = int(np.count_nonzero((coarse >> 4) == (((c - mn) >> shift) >> 4)))
    return "coarse" if in_bin * 128 <= len(x) else "dense"


def view(dfdb_mod, table, stages):
    dv = dfdb_mod.DFView(table)
    for st in stages:
        dv = dfdb_mod.selection(dv, dfdb_mod.jr(st[1], st[2], st[3]) if st[0] == "range" else st[1])
    return dv


def observed(ctx, dv):
    """(count, bitmap, indices, launches by profile key) of a fresh evaluation of the view's query"""
    ctx.profile(True)
    q = dv._query()
    q.reset()
    got = (q.count(), q.bitmap(), q.indices())
    prof = {k: ctx.profile_get(k)[0] for k in KEYS}
    ctx.profile(False)
    return got, prof


def numpy_answer(x, f, c, rows):
    """(count, bitmap, indices) of x OP c over the 1-based row range `rows` (None: every row)"""
    m = f(x, x.dtype.type(c))
    if rows is not None:
        keep = np.zeros(len(x), bool)
        keep[rows[0] - 1:rows[1]] = True
        m = m & keep
    bits = np.zeros(((len(x) + 63) // 64) * 64, np.uint8)
    bits[:len(x)] = m
    return int(m.sum()), np.packbits(bits, bitorder="little").view(np.uint64), np.flatnonzero(m).astype(np.int64) + 1


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def check_column(dfdb_mod, ctx, x, consts, modes):
    """every operator and constant, fresh and behind a range stage, under each scan_coarse mode: the answers against scan_image = 0 and numpy, the form that ran"""
    from dfdb import ir
    n = len(x)
    unsigned = x.dtype == np.uint64
    before = image_bytes(ctx)
    t = dfdb_mod.DFTable.from_columns({"x": x}, block_size=65536)
    lo = max(1, n // 3)
    hi = min(n, lo + 2000)
    try:
        for c in consts:
            k = ir.const(c, ir.U64) if unsigned else ir.const(c)
            for name, f in OPS.items():
                for rows in (None, (lo, hi)):
                    pred = ("pred", f(ir.col(0), k))
                    dv = view(dfdb_mod, t, [pred] if rows is None else [("range", rows[0], 1, rows[1]), pred])
                    want = numpy_answer(x, f, c, rows)
                    ctx.set_option("scan_image", 0)
                    flat, prof0 = observed(ctx, dv)
                    ctx.set_option("scan_image", 2)
                    what = (str(x.dtype), n, name, c, rows)
                    assert prof0["scan_image"] == 0 and prof0["scan_cmp"] == 1 and all(prof0[key] == 0 for key in FORMS["image"]), (what, prof0)
                    assert same(flat, want), what
                    for mode in modes:
                        ctx.set_option("scan_coarse", mode)
                        got, prof = observed(ctx, dv)
                        ctx.set_option("scan_coarse", 1)
                        form = expected_form(x, c, mode)
                        assert prof["scan_image"] == 1 and prof["scan_cmp"] == 0, (what, mode, prof)
                        assert {key: prof[key] for key in FORMS[form]} == FORMS[form], (what, mode, form, prof)
                        assert same(got, flat) and same(got, want), (what, mode, form)
        assert image_bytes(ctx) - before >= n * 6            # the image and its coarse copy, made once
    finally:
        t.close()
    assert image_bytes(ctx) == before


def spread_column(n, rng):
    """uniform in [0, 1e6) with the minimum and the maximum forced in (n >= 2: shift = 4), and rows inside and beside the bucket of K16"""
    x = rng.integers(0, 1_000_000, n).astype(np.int64)
    if n > 16:
        at = rng.choice(n, min(n // 2, 24), replace=False)
        x[at] = K16 + rng.integers(-2, 18, len(at))
    x[0] = 0
    if n > 1:
        x[-1] = 999_999
    return x


K16 = 31250 * 16          # the first value of a 16-wide bucket of the spread column (min 0, shift 4)
SPREAD_CONSTS = [K16 - 1, K16, K16 + 1, K16 + 15, 0, 999_999, -1, 1_000_000]


def test_spread_values_take_the_coarse_kernel_and_refine_exactly(dfdb_mod, coarse_ctx):
    """(a) values over [0, 1e6), shift 4: constants at the first, second and last value of a bucket and the last of the one before, at the minimum (cc = 0 with
    n % 8 != 0: the zero-filled rows past the end equal cc and must not be refined or counted), at the maximum, and one outside on either side (the 4-byte
    form).  Under scan_coarse = 2 a constant in range runs the coarse kernel at every size (one row: min == max, the exact form); the largest size also runs
    under the default, where the guard passes: a bucket bin holds about 1/3906 of the rows"""
    for n in SIZES:
        x = spread_column(n, np.random.default_rng(n))
        if n > 1:
            assert all(expected_form(x, c, 2) == "coarse" for c in SPREAD_CONSTS[:6])
            assert all(expected_form(x, c, 2) == "image" for c in SPREAD_CONSTS[6:])
        else:
            assert expected_form(x, 0, 2) == "exact"
        check_column(dfdb_mod, coarse_ctx, x, SPREAD_CONSTS, (2, 1) if n == SIZES[-1] else (2,))
    assert all(expected_form(x, c, 1) == "coarse" for c in SPREAD_CONSTS[:6])      # (the last column: the default took the coarse kernel there)


@pytest.mark.parametrize("kind", ["i", "u"])
def test_span_below_65536_takes_the_exact_two_byte_scan(dfdb_mod, coarse_ctx, kind):
    """(b) shift 0: the coarse value is the biased exact value, the shipped 2-byte scan answers every operator with no refinement — negative Int64 values
    included, and `==` on a column where half the rows equal the constant"""
    for n in SIZES:
        rng = np.random.default_rng(100 + n)
        if kind == "i":
            x = rng.integers(-30_000, 30_000, n).astype(np.int64)
            c = -12_345
        else:
            x = rng.integers(1_000, 60_000, n).astype(np.uint64)
            c = 40_000
        x[rng.random(n) < 0.5] = c
        x[0] = c
        consts = [c, int(x.min()), int(x.max()), int(x.min()) - 1, int(x.max()) + 1]
        assert all(expected_form(x, k, 1) == "exact" for k in consts[:3]) and all(expected_form(x, k, 1) == "image" for k in consts[3:])
        check_column(dfdb_mod, coarse_ctx, x, consts, (1,))


@pytest.mark.parametrize("kind", ["i", "u"])
def test_full_range_column_refines_every_row_when_forced_and_is_refused_by_the_guard(dfdb_mod, coarse_ctx, kind):
    """(c) the type's limits present (shift 16) and the bulk of the rows in the constant's bucket: under scan_coarse = 2 every such row is refined and the
    answers stay exact; under the default the guard refuses (scan_image.coarse_dense, one launch under scan_image, none under scan_cmp) and the 4-byte scan runs"""
    for n in SIZES:
        rng = np.random.default_rng(200 + n)
        if kind == "i":
            x = rng.integers(-50, 50, n).astype(np.int64)
            x[0] = I32_MIN
            if n > 1:
                x[-1] = I32_MAX
            if n > 2:
                x[1] = 7
            consts = [7, -3, I32_MIN, I32_MAX]
        else:
            x = rng.integers(0, 100, n).astype(np.uint64)
            x[0] = U32_MAX
            if n > 1:
                x[-1] = 0
            if n > 2:
                x[1] = 40
            consts = [40, 0, U32_MAX]
        if n > 2:
            assert expected_form(x, consts[0], 2) == "coarse" and expected_form(x, consts[0], 1) == "dense"
        check_column(dfdb_mod, coarse_ctx, x, consts, (2, 1))


def test_coarse_copy_lives_and_goes_with_the_image(oracle, dfdb_mod, coarse_ctx, tmp_path):
    """(d) the coarse copy is counted under scan_image_bytes and `decoded` beside the image (6 bytes per row together), built by one launch under its own key
    right behind the image's one, released on dfdb_table_unload and on close, rebuilt after a reload; scan_coarse = 0 leaves the 4-byte image as it was"""
    from dfdb import ir
    from dfdb import _native as N
    ctx = coarse_ctx
    n = 2 * 65536 + 77
    x = spread_column(n, np.random.default_rng(9))
    want = np.flatnonzero(x >= K16).astype(np.int64) + 1
    p = Pair(oracle, dfdb_mod, {"x": x}, via_files=str(tmp_path / "tb"))
    before = image_bytes(ctx)
    try:
        dv = view(dfdb_mod, p.d, [("pred", ir.col(0) >= K16)])
        got, prof = observed(ctx, dv)
        assert prof["scan_image.build"] == 1 and prof["scan_image.coarse_build"] == 1 and prof["scan_image"] == 1 and prof["scan_image.coarse"] == 1, prof
        assert image_bytes(ctx) - before >= n * 6 and p.d.resident_bytes("x")["decoded"] >= n * 14
        assert np.array_equal(got[2], want)
        got, prof = observed(ctx, dv)                      # made once: the next scan builds nothing
        assert prof["scan_image.build"] == 0 and prof["scan_image.coarse_build"] == 0 and prof["scan_image.coarse"] == 1, prof
        N.check(N.load().dfdb_table_unload(p.d._h, None, 0))
        assert image_bytes(ctx) == before and p.d.resident_bytes("x")["decoded"] == 0
        p.d.load()
        got, prof = observed(ctx, dv)
        assert prof["scan_image.build"] == 1 and prof["scan_image.coarse_build"] == 1 and prof["scan_image.coarse"] == 1, prof
        assert image_bytes(ctx) - before >= n * 6
        assert np.array_equal(got[2], want)
    finally:
        p.d.close()
    assert image_bytes(ctx) == before
    ctx.set_option("scan_coarse", 0)
    t = dfdb_mod.DFTable.from_columns({"x": x}, block_size=65536)
    try:
        dv = view(dfdb_mod, t, [("pred", ir.col(0) >= K16)])
        got, prof = observed(ctx, dv)
        assert prof["scan_image.build"] == 1 and prof["scan_image.coarse_build"] == 0 and prof["scan_image"] == 1, prof
        assert all(prof[key] == 0 for key in FORMS["image"]), prof
        assert n * 4 <= image_bytes(ctx) - before < n * 6 and np.array_equal(got[2], want)
    finally:
        t.close()
    assert image_bytes(ctx) == before


def test_no_room_for_the_image_or_for_the_coarse_copy_is_noted_and_the_scan_still_answers(dfdb_mod, coarse_ctx):
    """(e) ctx option hbm_budget_mb (whole megabytes) leaves room beside the loaded column (a) for less than the image: one scan_image.no_room, nothing built or
    held, the flat scan_cmp answers, and the column is not tried again; (b) for the image but not the coarse copy behind it: one scan_image.coarse_no_room, the
    scan runs under scan_image with none of the coarse notes and 4 to 6 bytes per row are held.  The row count is taken from what the loaded table reports as
    resident: the first candidate for which a whole number of megabytes falls into both windows (image = 4 B/row + 256, coarse copy = 2 B/row + 256)."""
    from dfdb import ir
    ctx = coarse_ctx
    keys = KEYS + ("scan_image.no_room", "scan_image.coarse_no_room")
    mb = 1 << 20

    def whole_mb(held, lo, hi):
        """the budget in MB that leaves at least lo and fewer than hi bytes beside `held` (None: no whole number of megabytes does)"""
        b = -(-(held + lo) // mb)
        return b if b * mb - held < hi else None

    def scan(dv):
        ctx.profile(True)
        q = dv._query()
        q.reset()
        got = (q.count(), q.bitmap(), q.indices())
        prof = {k: ctx.profile_get(k)[0] for k in keys}
        ctx.profile(False)
        return got, prof

    before = image_bytes(ctx)
    tried = []
    for n in range(300_000, 360_000, 10_000):
        x = spread_column(n, np.random.default_rng(n))
        t = dfdb_mod.DFTable.from_columns({"x": x}, block_size=65536)
        try:
            held = sum(t.resident_bytes().values())
            image, coarse = 4 * n + 256, 2 * n + 256
            budget_a, budget_b = whole_mb(held, 0, image), whole_mb(held, image, image + coarse)
            tried.append((n, held, budget_a, budget_b))
            if budget_a is None or budget_b is None:
                continue
            dv = view(dfdb_mod, t, [("pred", ir.col(0) >= K16)])
            want = numpy_answer(x, operator.ge, K16, None)
            try:
                ctx.set_option("hbm_budget_mb", budget_a)
                got, prof = scan(dv)
                assert prof["scan_image.no_room"] == 1 and prof["scan_image.coarse_no_room"] == 0, prof
                assert prof["scan_image"] == 0 and prof["scan_image.build"] == 0 and prof["scan_image.coarse_build"] == 0 and prof["scan_cmp"] == 1, prof
                assert image_bytes(ctx) == before and same(got, want)
                got, prof = scan(dv)                       # refused once: not tried again while the column stays as it is
                assert prof["scan_image.no_room"] == 0 and prof["scan_image"] == 0 and prof["scan_cmp"] == 1 and same(got, want), prof
            finally:
                ctx.set_option("hbm_budget_mb", 0)
        finally:
            t.close()
        assert image_bytes(ctx) == before
        t = dfdb_mod.DFTable.from_columns({"x": x}, block_size=65536)
        try:
            assert sum(t.resident_bytes().values()) == held
            dv = view(dfdb_mod, t, [("pred", ir.col(0) >= K16)])
            try:
                ctx.set_option("hbm_budget_mb", budget_b)
                got, prof = scan(dv)
                assert prof["scan_image.coarse_no_room"] == 1 and prof["scan_image.no_room"] == 0, prof
                assert prof["scan_image.build"] == 1 and prof["scan_image.coarse_build"] == 0 and prof["scan_image"] == 1 and prof["scan_cmp"] == 0, prof
                assert all(prof[key] == 0 for key in FORMS["image"]), prof
                assert n * 4 <= image_bytes(ctx) - before < n * 6 and same(got, want)
            finally:
                ctx.set_option("hbm_budget_mb", 0)
        finally:
            t.close()
        assert image_bytes(ctx) == before
        return
    pytest.fail(f"no row count with a whole-megabyte budget for both cases: {tried}")
