"""The 4-byte scan image of Int64 / UInt64 columns whose values fit 32 bits (csrc/scan_image.hpp, k_image.hip, scan_image.cpp run_image_scan): a lone
`col OP const` scan reads the truncated copy through the shipped 4-byte scan kernel.  Every answer must be the flat column's bit for bit, and the oracle's;
the image must exist only for the columns, terms and constants it is valid for, be built when the options say, and go when the column's contents go."""
import operator

import numpy as np
import pytest

from helpers import Pair, apply_stages, assert_same

pytestmark = pytest.mark.gpu

OPS = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}
I32_MIN, I32_MAX, U32_MAX = -(1 << 31), (1 << 31) - 1, (1 << 32) - 1
MIN_ROWS_DEFAULT = 1 << 24
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 - 1, 3 * 4096 + 1, 65536 + 17]
KEYS = ("scan_cmp", "scan_image", "scan_image.build", "scan_image.misfit")


@pytest.fixture()
def image_ctx(ctx):
    """the session's context with the image built at the first eligible scan of any size; the library's defaults afterwards"""
    ctx.set_option("scan_image", 2)
    ctx.set_option("scan_image_min_rows", 1)
    try:
        yield ctx
    finally:
        ctx.profile(False)
        ctx.set_option("scan_image", 1)
        ctx.set_option("scan_image_min_rows", MIN_ROWS_DEFAULT)


def image_bytes(ctx):
    return ctx.profile_get("scan_image_bytes")[0]


def column(kind, n, rng):
    """values that fit the image type, its limits mixed in"""
    if kind == "i":
        x = rng.integers(-50, 50, n).astype(np.int64)
        edge = np.array([I32_MIN, -1, 0, I32_MAX], np.int64)
    else:
        x = rng.integers(0, 100, n).astype(np.uint64)
        edge = np.array([0, U32_MAX], np.uint64)
    at = rng.integers(0, n, min(n, 12))
    x[at] = edge[rng.integers(0, len(edge), len(at))]
    return x


def constants(kind):
    """[(constant, representable in the image type)]: the type's limits, one inside them, outside on every side there is"""
    if kind == "i":
        return [(I32_MIN, True), (I32_MAX, True), (7, True), (I32_MAX + 1, False), (I32_MIN - 1, False)]
    return [(0, True), (U32_MAX, True), (40, True), (U32_MAX + 1, False)]


def observed(ctx, dv):
    """(count, bitmap, indices, launches by profile key) of a fresh evaluation of the view's query"""
    ctx.profile(True)
    q = dv._query()
    q.reset()
    got = (q.count(), q.bitmap(), q.indices())
    prof = {k: ctx.profile_get(k)[0] for k in KEYS}
    ctx.profile(False)
    return got, prof


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("kind", ["i", "u"])
def test_image_scan_equals_flat_scan_and_oracle(oracle, dfdb_mod, image_ctx, kind):
    """every operator, constants at and around the image type's limits, as a fresh mask and after a range stage (and_existing), at row counts around one
    word, one tile, one four-tile group and several groups: count, bitmap and indices under scan_image = 0 and with the image agree bit for bit, and with the
    oracle; a representable constant runs the image scan, one outside the type's range the flat scan"""
    for n in SIZES:                  # (one test per dtype: the thirteen row counts together take well under a second)
        image_scan_cases(oracle, dfdb_mod, image_ctx, kind, n)


def image_scan_cases(oracle, dfdb_mod, ctx, kind, n):
    from dfdb import ir
    rng = np.random.default_rng(n * 7 + (kind == "u"))
    x = column(kind, n, rng)
    p = Pair(oracle, dfdb_mod, {"x": x})
    before = image_bytes(ctx)
    lo = max(1, n // 3)
    hi = min(n, lo + 2000)
    try:
        for c, fits in constants(kind):
            k = ir.const(c, ir.U64) if kind == "u" else ir.const(c)
            for name, f in OPS.items():
                for stages in ([("pred", f(ir.col(0), k))], [("range", lo, 1, hi), ("pred", f(ir.col(0), k))]):
                    ov, dv = apply_stages(p, stages)
                    ctx.set_option("scan_image", 0)
                    flat, prof0 = observed(ctx, dv)
                    ctx.set_option("scan_image", 2)
                    img, prof = observed(ctx, dv)
                    what = (kind, n, name, c, len(stages))
                    assert prof0["scan_image"] == 0 and prof0["scan_image.build"] == 0 and prof0["scan_cmp"] == 1, (what, prof0)
                    assert same(flat, img), what
                    if fits:
                        assert prof["scan_image"] == 1 and prof["scan_cmp"] == 0, (what, prof)
                    else:
                        assert prof["scan_image"] == 0 and prof["scan_cmp"] > 0, (what, prof)
                    if len(stages) == 1:
                        want = np.flatnonzero(f(x, x.dtype.type(c)))          # (every constant here is a value of the COLUMN's type)
                        assert np.array_equal(img[2], want.astype(np.int64) + 1), what
                    assert_same(p, ov, dv)
        assert image_bytes(ctx) - before >= n * 4            # one image, made once
    finally:
        p.d.close()
    assert image_bytes(ctx) == before


def test_column_that_does_not_fit_gets_no_image(oracle, dfdb_mod, image_ctx):
    """one value of 2^31 (Int64) / 2^32 (UInt64) in the LAST row: the build finds it, the image is released, the column is never tried again, answers unchanged"""
    for kind in ("i", "u"):
        misfit_cases(oracle, dfdb_mod, image_ctx, kind)


def misfit_cases(oracle, dfdb_mod, ctx, kind):
    from dfdb import ir
    n = 3 * 4096 + 1
    x = column(kind, n, np.random.default_rng(5))
    x[-1] = (1 << 31) if kind == "i" else (1 << 32)
    p = Pair(oracle, dfdb_mod, {"x": x})
    before = image_bytes(ctx)
    k = ir.const(7, ir.U64) if kind == "u" else ir.const(7)
    try:
        for rnd in range(2):
            for name, f in OPS.items():
                ov, dv = apply_stages(p, [("pred", f(ir.col(0), k))])
                got, prof = observed(ctx, dv)
                first = rnd == 0 and name == "=="
                assert prof["scan_image.build"] == (1 if first else 0) and prof["scan_image.misfit"] == (1 if first else 0), (kind, name, rnd, prof)
                assert prof["scan_image"] == 0 and prof["scan_cmp"] == 1, (kind, name, rnd, prof)
                assert image_bytes(ctx) == before
                assert np.array_equal(got[2], np.flatnonzero(f(x, x.dtype.type(7))).astype(np.int64) + 1)
                assert_same(p, ov, dv)
    finally:
        p.d.close()


def test_columns_and_terms_that_take_the_flat_path(oracle, dfdb_mod, image_ctx):
    """a nullable Int64 column and a Float64 column get no image; a term whose column the scan captures for the projection (materialize hint) reads the flat
    column although its column has an image; a second comparison of the same column and a transformed column do too"""
    from dfdb import ir
    ctx = image_ctx
    n = 4096 + 33
    rng = np.random.default_rng(11)
    a = rng.integers(-50, 50, n).astype(np.int64)
    m = np.ma.masked_array(rng.integers(-50, 50, n).astype(np.int64), mask=rng.random(n) < 0.2)
    x = rng.integers(-50, 50, n).astype(np.float64)
    p = Pair(oracle, dfdb_mod, {"a": a, "m": m, "x": x})
    before = image_bytes(ctx)
    try:
        for pred in (ir.coalesce(ir.col(1) > 3, False), ir.col(2) > 3.0):
            ov, dv = apply_stages(p, [("pred", pred)])
            _, prof = observed(ctx, dv)
            assert prof["scan_image"] == 0 and prof["scan_image.build"] == 0 and image_bytes(ctx) == before, prof
            assert_same(p, ov, dv)
        ov, dv = apply_stages(p, [("pred", ir.col(0) > 3)], proj=[("a", ir.col(0))])
        _, prof = observed(ctx, dv)
        assert prof["scan_image"] == 1 and prof["scan_image.build"] == 1 and image_bytes(ctx) > before, prof
        ctx.profile(True)
        q = dv._query()
        q.reset()
        q.hint_materialize(True)
        assert q.count() == int((a > 3).sum())
        prof = {k: ctx.profile_get(k)[0] for k in KEYS}
        ctx.profile(False)
        assert prof["scan_image"] == 0 and prof["scan_cmp"] == 1, prof
        assert_same(p, ov, dv)
        for pred in ((ir.col(0) > -20) & (ir.col(0) < 20), ir.col(0) % 7 == 0):
            ov, dv = apply_stages(p, [("pred", pred)])
            _, prof = observed(ctx, dv)
            assert prof["scan_image"] == 0, prof
            assert_same(p, ov, dv)
    finally:
        p.d.close()
    assert image_bytes(ctx) == before


def test_auto_mode_builds_at_the_second_scan_and_never_below_the_row_threshold(oracle, dfdb_mod, image_ctx):
    """scan_image = 1 (the default): the first single-term scan of a column is the flat one, the second builds the image, from then on the image is read;
    a table below scan_image_min_rows never gets one"""
    from dfdb import ir
    ctx = image_ctx
    n = 4096 + 5
    x = np.random.default_rng(3).integers(-1000, 1000, n).astype(np.int64)
    ctx.set_option("scan_image", 1)
    before = image_bytes(ctx)
    p = Pair(oracle, dfdb_mod, {"x": x})
    try:
        seen = []
        for c in (10, 20, 30, 40):
            ov, dv = apply_stages(p, [("pred", ir.col(0) > c)])
            got, prof = observed(ctx, dv)
            assert got[0] == int((x > c).sum())
            seen.append((prof["scan_cmp"], prof["scan_image.build"], prof["scan_image"]))
        assert seen == [(1, 0, 0), (0, 1, 1), (0, 0, 1), (0, 0, 1)], seen
        assert_same(p, ov, dv)
        assert image_bytes(ctx) - before >= n * 4
    finally:
        p.d.close()
    ctx.set_option("scan_image_min_rows", n + 1)
    p = Pair(oracle, dfdb_mod, {"x": x})
    try:
        for c in (10, 20, 30, 40):
            ov, dv = apply_stages(p, [("pred", ir.col(0) > c)])
            _, prof = observed(ctx, dv)
            assert (prof["scan_cmp"], prof["scan_image.build"], prof["scan_image"]) == (1, 0, 0), prof
        assert image_bytes(ctx) == before
    finally:
        p.d.close()


def test_image_goes_with_the_column_and_is_rebuilt_after_a_reload(oracle, dfdb_mod, image_ctx, tmp_path):
    """dfdb_table_unload releases the image with the column; after a reload the next scan builds it again from the reloaded contents"""
    from dfdb import ir
    from dfdb import _native as N
    ctx = image_ctx
    n = 2 * 65536 + 77
    x = column("i", n, np.random.default_rng(9))
    p = Pair(oracle, dfdb_mod, {"x": x}, via_files=str(tmp_path / "tb"))
    before = image_bytes(ctx)
    try:
        ov, dv = apply_stages(p, [("pred", ir.col(0) >= 7)])
        _, prof = observed(ctx, dv)
        assert prof["scan_image.build"] == 1 and prof["scan_image"] == 1 and image_bytes(ctx) - before >= n * 4, prof
        assert p.d.resident_bytes("x")["decoded"] >= n * 12
        assert_same(p, ov, dv)
        N.check(N.load().dfdb_table_unload(p.d._h, None, 0))
        assert image_bytes(ctx) == before and p.d.resident_bytes("x")["decoded"] == 0
        p.d.load()
        ov, dv = apply_stages(p, [("pred", ir.col(0) >= 7)])
        got, prof = observed(ctx, dv)
        assert prof["scan_image.build"] == 1 and prof["scan_image"] == 1 and image_bytes(ctx) - before >= n * 4, prof
        assert np.array_equal(got[2], np.flatnonzero(x >= 7).astype(np.int64) + 1)
        assert_same(p, ov, dv)
    finally:
        p.d.close()
    assert image_bytes(ctx) == before
