"""`s1 OP s2` over two String columns on the device (==, !=, <, <=, >, >=; Base.cmp on the bytes): the interpreter's H_STRCMP2 is the definition, k_str_pair the
kernel of a top-level conjunct, k_dict_pair the form of two dictionary columns.  The yardstick is the oracle through helpers (count, bitmap, indices and
materialized columns bit for bit); tests/test_str_pair_cpu.py pins the oracle to the four-line definition on `bytes`."""
import numpy as np
import pytest

import collections

from helpers import _engine_view, _oracle_view, apply_stages, assert_same
from str_pair_cases import IR_OPS, OPS, S, build, cmp, content_columns, expect

pytestmark = pytest.mark.gpu

BS = 65536
BIG = 65536 + 1025                      # two blocks, a tile boundary after the block boundary, a ragged last tile
NAMES = ("str_pair", "dict_pair", "interp_predicate", "jit_predicate", "interp_project", "jit_project")


@pytest.fixture(params=[0, 2], ids=["jit0", "jit2"])
def jit(ctx, request):
    """every case under the ahead-of-time interpreter and under its run-time compiled form"""
    ctx.set_option("jit", request.param)
    ctx.set_option("jit_min_rows", 0)
    yield request.param
    ctx.set_option("jit", 1)
    ctx.set_option("jit_min_rows", 1 << 22)


Form = collections.namedtuple("Form", "kernel jit")          # which form must answer a pair conjunct, and which form of the interpreter runs


@pytest.fixture(params=[1, 0], ids=["kernel", "interp"])
def kern(ctx, jit, request):
    """a pair conjunct through k_str_pair / k_dict_pair and through the interpreter's H_STRCMP2 (csrc/KNOBS.md: str_pair_kernel)"""
    ctx.set_option("str_pair_kernel", request.param)
    yield Form(request.param, jit)
    ctx.set_option("str_pair_kernel", 1)


def launches(ctx, fn):
    """launches by profile name while fn runs"""
    ctx.profile(True)
    before = [ctx.profile_get(k)[0] for k in NAMES]
    try:
        fn()
    finally:
        after = [ctx.profile_get(k)[0] for k in NAMES]
        ctx.profile(False)
    return {k: a - b for k, a, b in zip(NAMES, after, before)}


def assert_form(n, kern, form="str_pair", only_kernel=True):
    """n: launches by name.  kern.kernel = 1: the pair kernel `form` answered (and, with only_kernel, no interpreter program ran beside it); 0: no pair kernel
    ran and the interpreter answered — the ahead-of-time one under jit 0, the run-time compiled one under jit 2 (jit_min_rows is 0: every program is
    compiled, so an ahead-of-time launch there is a silent fallback)"""
    ahead, compiled = n["interp_predicate"], n["jit_predicate"]
    assert (compiled == 0) if kern.jit == 0 else (ahead == 0), n
    if kern.kernel:
        assert n[form] >= 1 and (not only_kernel or ahead + compiled == 0), n
    else:
        assert n["str_pair"] == 0 and n["dict_pair"] == 0 and (ahead if kern.jit == 0 else compiled) >= 1, n


def check(ctx, p, stages, proj=None, kern=None, form="str_pair", only_kernel=True):
    """the view equals the oracle's; with `kern` given, the form that answered the pair conjunct is the one it names"""
    ov, dv = apply_stages(p, stages, proj=proj)
    n = launches(ctx, lambda: assert_same(p, ov, dv))
    if kern is not None:
        assert_form(n, kern, form, only_kernel)
    return ov


def want_indices(op, a, b):
    return np.array([i + 1 for i in range(len(a)) if expect(op, a[i], b[i])], np.int64)


# ---------------------------------------------------------------- content, row counts, operators
@pytest.mark.parametrize("lean", [False, True], ids=["dense", "lean"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049, BIG])
def test_row_counts(oracle, dfdb_mod, ctx, jit, kern, n, lean):
    from dfdb import ir
    a, b = content_columns(n, lean)
    p = build(oracle, dfdb_mod, {"a": S(a), "b": S(b)}, block_size=BS)
    for op in ("==", "<"):
        ov = check(ctx, p, [("pred", IR_OPS[op](ir.col(0), ir.col(1)))], kern=kern)
        assert np.array_equal(ov.select_indices(), want_indices(op, a, b))             # the definition itself, beside the oracle
    p.d.close()


def test_through_files(oracle, dfdb_mod, ctx, jit, kern, tmp_path):
    """the oracle's writer (liblz4) wrote the table: the device LZ4 decode is in the path"""
    from dfdb import ir
    a, b = content_columns(BIG, True)
    p = build(oracle, dfdb_mod, {"a": S(a), "b": S(b)}, block_size=BS, via_files=str(tmp_path / "tb"))
    check(ctx, p, [("pred", ir.col(0) >= ir.col(1))], kern=kern)
    check(ctx, p, [("pred", ir.col(1) != ir.col(0))], kern=kern)
    p.d.close()


@pytest.mark.parametrize("op", list(OPS))
def test_six_operators_both_orders_and_a_column_against_itself(oracle, dfdb_mod, ctx, jit, kern, op):
    from dfdb import ir
    for lean in (False, True):
        a, b = content_columns(2049, lean)
        p = build(oracle, dfdb_mod, {"a": S(a), "b": S(b)}, block_size=BS)
        for l, r in ((0, 1), (1, 0), (0, 0)):
            ov = check(ctx, p, [("pred", IR_OPS[op](ir.col(l), ir.col(r)))], kern=kern)
            cols = (a, b)
            assert np.array_equal(ov.select_indices(), want_indices(op, cols[l], cols[r]))
        p.d.close()


def test_long_tiles_beside_short_ones(oracle, dfdb_mod, ctx, jit, kern):
    """tiles of 1024 rows of 40-byte strings (40 KB: more than any staging of a tile's bytes would hold, K5's 8 KB included) in column 1 only, in column 2
    only and in both, each between tiles of short strings: every row walks five 8-byte words, and the tile offsets of the two columns drift apart"""
    from dfdb import ir
    a, b = content_columns(7 * 1024 + 77, True)

    def long(i, k):
        return b"%039d" % (i % 7) + (b"x" if (i + k) % 3 else b"y")
    for t, (la, lb) in {1: (True, False), 3: (False, True), 5: (True, True)}.items():
        for i in range(t * 1024, (t + 1) * 1024):
            if la: a[i] = long(i, 0)
            if lb: b[i] = long(i, 1) if i % 5 else a[i]
    p = build(oracle, dfdb_mod, {"a": S(a), "b": S(b)}, block_size=BS)
    for op in ("==", "!=", "<", ">="):
        ov = check(ctx, p, [("pred", IR_OPS[op](ir.col(0), ir.col(1)))], kern=kern)
        assert np.array_equal(ov.select_indices(), want_indices(op, a, b))
    p.d.close()


# ---------------------------------------------------------------- missing values
def with_missing(n, left, right):
    a, b = content_columns(n, True)
    rows = [r for r in (0, 63, 64, 1023, n - 1) if r < n]
    for k, r in enumerate(rows):
        if left and (not right or k % 3 != 1): a[r] = None
        if right and (not left or k % 3 != 0): b[r] = None
    return a, b


@pytest.mark.parametrize("left,right", [(True, False), (False, True), (True, True)], ids=["left", "right", "both"])
def test_missing_rows(oracle, dfdb_mod, ctx, jit, kern, left, right):
    from dfdb import ir
    n = 2049
    a, b = with_missing(n, left, right)
    p = build(oracle, dfdb_mod, {"a": S(a, left), "b": S(b, right), "k": np.arange(n, dtype=np.int64)}, block_size=BS)
    for op in ("==", "!=", "<=", ">"):
        e = IR_OPS[op](ir.col(0), ir.col(1))
        assert p.d.expr_dtype(e) == ir.BOOL | ir.NULLABLE
        ov = check(ctx, p, [("pred", ir.coalesce(e, False))], kern=kern)              # the kernel form: a missing row selects nothing
        assert np.array_equal(ov.select_indices(), want_indices(op, a, b))
        check(ctx, p, [], proj=[("r", e), ("k", ir.col(2))])                          # a projected Union{Bool,Missing} column: flags and values
        check(ctx, p, [("pred", ir.col(2) % 3 != 1)], proj=[("r", e)])
    # the bare nullable predicate: refused by both sides, with the same exception class
    errs = []
    for f in (_oracle_view, _engine_view):
        with pytest.raises(Exception) as ei:
            f(p, [("pred", ir.col(0) < ir.col(1))], None)
        errs.append(type(ei.value).__name__)
    assert errs[0] == errs[1], errs
    p.d.close()


# ---------------------------------------------------------------- composition
@pytest.fixture(scope="module")
def three(oracle, dfdb_mod, ctx):
    n = 5 * 1024 + 300
    a, b = content_columns(n, True)
    c = [b[(i * 7 + 3) % n] for i in range(n)]
    rng = np.random.default_rng(3)
    x = rng.integers(0, 10, n).astype(np.int64)
    x[2048:4096] = 0                                                                   # `x > 0` leaves two whole tiles empty
    p = build(oracle, dfdb_mod, {"a": S(a), "b": S(b), "c": S(c), "x": x, "g": (np.arange(n) % 5).astype(np.int64)}, block_size=BS)
    yield p, a, b, c, x
    p.d.close()


def test_composition(ctx, jit, kern, three):
    from dfdb import ir
    p, a, b, c, x = three
    A, B, Cc, X = ir.col(0), ir.col(1), ir.col(2), ir.col(3)
    check(ctx, p, [("range", 100, 3, 5000), ("pred", A == B)], kern=kern)                       # after a range stage: AND_EXISTING
    check(ctx, p, [("pred", X > 0), ("range", 1, 1, 3000), ("pred", A < B)], kern=kern, only_kernel=False)      # after a predicate stage that emptied tiles
    check(ctx, p, [("pred", A >= B), ("range", 5, 2, 900)], kern=kern)                           # before a second stage
    check(ctx, p, [("pred", (A == B) & (X > 4))], kern=kern)                                     # one stage, two conjuncts
    check(ctx, p, [("pred", (A == B) & (B < Cc))], kern=kern)                                    # three String columns
    check(ctx, p, [("pred", (A != B) & (X + X > 6))], kern=kern, only_kernel=False)              # beside a generic conjunct
    for e in ((A == B) | (X > 7), ~(A < B)):                                                     # under | and !: the interpreter's, whatever the knob says
        check(ctx, p, [("pred", e)], kern=Form(0, jit))
    check(ctx, p, [("pred", A <= B)], proj=[("a", A), ("x", X), ("same", A == B)], kern=kern)    # a pair column projected and materialized, a computed column
    check(ctx, p, [("pred", A == "ab"), ("pred", A == B)], proj=[("a", A)], kern=kern)           # beside K5's constant term (its projection shortcut)


def test_groupreduce_over_a_pair_selected_view(dfdb_mod, ctx, jit, kern, three):
    from dfdb import ir
    p, a, b, c, x = three
    v = dfdb_mod.DFView(p.d)[ir.col(0) < ir.col(1), dfdb_mod.ALL]
    res = {}
    n = launches(ctx, lambda: res.update(r=dfdb_mod.groupreduce(v, "g", "x", "sum")))
    assert_form(n, kern)
    sel = np.array([cmp(p_, q_) < 0 for p_, q_ in zip(a, b)])
    g = np.arange(len(a)) % 5
    got = {int(k): (int(cn), int(s)) for k, cn, s in zip(res["r"]["g"].to_numpy(), res["r"]["count"].to_numpy(), res["r"]["sum"].to_numpy())}
    assert got == {k: (int((sel & (g == k)).sum()), int(x[sel & (g == k)].sum())) for k in range(5)}
    assert dfdb_mod.DFView(p.d)[ir.col(0) < ir.col(1), "x"].sum() == int(x[sel].sum())


def test_through_dfcolumn_operators(dfdb_mod, ctx, jit, kern, three):
    """the mirror's front end: the comparison operators between two String DFColumns (api.py DFColumn._bc) build the same expression — as a selection,
    as a computed Bool column, and summed"""
    p, a, b, c, x = three
    t = p.d
    for op in OPS:
        res = {}
        n = launches(ctx, lambda: res.update(i=t[IR_OPS[op](t.a, t.b), dfdb_mod.ALL]._query().indices()))
        assert_form(n, kern)
        assert np.array_equal(res["i"], want_indices(op, a, b))
    same = t.a == t.c
    holds = np.array([expect("==", p_, q_) for p_, q_ in zip(a, c)])
    assert np.array_equal(np.asarray(dfdb_mod.materialize(same), dtype=bool), holds)
    assert same.sum() == int(holds.sum())
    assert dfdb_mod.nrow(t[(t.a >= t.b) & (t.x > 4), ["x"]]) == sum(1 for p_, q_, v in zip(a, b, x) if p_ >= q_ and v > 4)


# ---------------------------------------------------------------- dictionaries
@pytest.mark.parametrize("distinct", [3, 300, 9000])
def test_two_dictionary_columns(oracle, dfdb_mod, ctx, jit, kern, distinct):
    """both columns with a dictionary, the two sets overlapping partly (9000 + 9000 entries: the rank tables stay in device memory instead of LDS)"""
    from dfdb import ir
    rng = np.random.default_rng(distinct)
    n = 20_000

    def word(k):
        return (b"%c%c" % (97 + k % 5, 0x7f + k % 3)) * (k % 4) + b"%d" % k
    a = [word(int(k)) for k in rng.integers(0, distinct, n)]
    b = [word(int(k)) for k in rng.integers(distinct // 3, distinct + distinct // 3, n)]
    a[:distinct] = [word(k) for k in range(distinct)]
    b[:distinct] = [word(k + distinct // 3) for k in range(distinct)]
    for i in range(distinct, n, 3):
        b[i] = a[i]
    p = build(oracle, dfdb_mod, {"a": S(a), "b": S(b), "x": np.arange(n, dtype=np.int64)}, block_size=BS)
    flat = {}
    for op in OPS:
        flat[op] = check(ctx, p, [("pred", IR_OPS[op](ir.col(0), ir.col(1)))], kern=kern).select_indices()
        assert np.array_equal(flat[op], want_indices(op, a, b))
    assert p.d.build_dictionary("a", 65535) == len(set(a))
    for op in ("==", "<"):                                                             # one column only with a dictionary: the byte kernel, the same answer
        ov = check(ctx, p, [("pred", IR_OPS[op](ir.col(0), ir.col(1)))], kern=kern)
        assert np.array_equal(ov.select_indices(), flat[op])
        ov = check(ctx, p, [("pred", IR_OPS[op](ir.col(1), ir.col(0)))], kern=kern)
    assert p.d.build_dictionary("b", 65535) == len(set(b))
    for op in OPS:
        ov = check(ctx, p, [("pred", IR_OPS[op](ir.col(0), ir.col(1)))], kern=kern, form="dict_pair")
        assert np.array_equal(ov.select_indices(), flat[op])
    check(ctx, p, [("pred", ir.col(2) % 7 < 3), ("pred", ir.col(1) > ir.col(0))], proj=[("a", ir.col(0)), ("b", ir.col(1))], kern=kern, form="dict_pair")
    p.d.close()


# ---------------------------------------------------------------- placement
@pytest.fixture(scope="module")
def placed(oracle, dfdb_mod, ctx, tmp_path_factory):
    """the BIG table resident (from files) with its answers, and its path"""
    from dfdb import ir
    a, b = content_columns(BIG, True)
    path = str(tmp_path_factory.mktemp("str_pair") / "tb")
    p = build(oracle, dfdb_mod, {"a": S(a), "b": S(b), "x": (np.arange(BIG) % 11).astype(np.int64)}, block_size=4096, via_files=path)
    exprs = {"==": ir.col(0) == ir.col(1), "<": ir.col(0) < ir.col(1)}
    want = {k: want_indices(k, a, b) for k in exprs}
    for k, e in exprs.items():
        assert np.array_equal(dfdb_mod.DFView(p.d)[e, dfdb_mod.ALL]._query().indices(), want[k])
    yield p, path, exprs, want
    p.d.close()


def test_compressed_only_neighbours(oracle, dfdb_mod, ctx, jit, kern):
    """the numeric column of the query holds its LZ4 blocks only: the pair conjunct beside K7's fused scan and in one interpreter program with a decoded column.
    A String column cannot itself be held compressed-only — compress_column takes fixed-width columns and the load path keeps the bytes of a String column
    decoded — so the compressed-only placement a pair expression can meet is that of the columns beside it"""
    from dfdb import ir
    a, b = content_columns(BIG, True)
    p = build(oracle, dfdb_mod, {"a": S(a), "b": S(b), "x": (np.arange(BIG) % 11).astype(np.int64)}, block_size=4096)
    p.d.compress_column("x", 2)
    check(ctx, p, [("pred", (ir.col(0) == ir.col(1)) & (ir.col(2) > 4))], proj=[("x", ir.col(2)), ("b", ir.col(1))], kern=kern)
    check(ctx, p, [("pred", (ir.col(0) < ir.col(1)) | (ir.col(2) * 2 > 19))], proj=[("x", ir.col(2))])
    p.d.close()


def test_out_of_core_streamed_and_sharded(dfdb_mod, ctx, jit, kern, placed):
    from dfdb import group as G, _native as NAT
    p, path, exprs, want = placed
    # out of core through the ordinary entry points: a context whose budget holds nothing
    c2 = dfdb_mod.Context()
    for k, v in (("hbm_budget_mb", 1), ("ooc_chunk_blocks", 3), ("jit", jit), ("jit_min_rows", 0), ("str_pair_kernel", kern.kernel)):
        c2.set_option(k, v)
    lazy = dfdb_mod.open_table(path, load=False, ctx=c2)
    try:
        for k, e in exprs.items():
            v = dfdb_mod.DFView(lazy)[e, ["x", "a"]]
            # (the chunks run on contexts of the stream's own, which no entry point hands out: which form ran there cannot be read, only that the answer holds)
            assert np.array_equal(v._query().indices(), want[k]) and dfdb_mod.nrow(v) == len(want[k])
            got = dfdb_mod.materialize(v)
            assert np.array_equal(got["x"].to_numpy(), (want[k] - 1) % 11)
            assert not lazy.resident(0) and not lazy.resident(1)
        # the explicit stream
        with dfdb_mod.stream(dfdb_mod.DFView(lazy)[exprs["<"], ["x"]], 2) as s:
            idx = [part.indices() for part in s]
        assert np.array_equal(np.concatenate(idx), want["<"])
    finally:
        lazy.close(); c2.close()
    # three block-range shards on one device
    g = G.Group.create([0, 0, 0], NAT.EXCHANGE_HOST)
    try:
        for k, v in (("jit", jit), ("jit_min_rows", 0), ("str_pair_kernel", kern.kernel)):
            g.set_option(k, v)
        gt = G.GroupTable.open(g, path)
        shards = [g.ctx(i) for i in range(3)]
        for c in shards:
            c.profile(True)
        for k, e in exprs.items():
            ref = dfdb_mod.DFView(p.d)[e, ["x"]]
            gv = dfdb_mod.DFView(gt.view().table, ref.projection, ref.selection)
            assert G.gnrow(gv) == len(want[k]) and np.array_equal(G.gindices(gv), want[k])
            assert np.array_equal(G._gq(gv).materialize()[0], (want[k] - 1) % 11)
        for c in shards:                                                                # every shard answered in the form the knob names
            assert_form({name: c.profile_get(name)[0] for name in NAMES}, kern)
            c.profile(False)
        gt.close()
    finally:
        g.close()


# ---------------------------------------------------------------- differential fuzz
ALPHABET = [b"a", b"b", b"\0", b"\x7f", b"\xc3", b"\xbf"]


def fuzz_columns(seed):
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.integers(1500, 5001))

    def draw():
        return b"".join(ALPHABET[int(k)] for k in rng.integers(0, 6, int(rng.integers(0, 25))))
    a = [draw() for _ in range(n)]
    b = [a[i] if rng.random() < 1 / 3 else draw() for i in range(n)]
    # (independent draws are ordered either way with equal probability: about a third of the rows each of <, =, >)
    na, nb = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    if na:
        for i in rng.integers(0, n, n // 20): a[int(i)] = None
    if nb:
        for i in rng.integers(0, n, n // 20): b[int(i)] = None
    return rng, n, a, b, na, nb


@pytest.mark.parametrize("seed", range(40))
def test_fuzz(oracle, dfdb_mod, ctx, jit, kern, seed):
    from dfdb import ir
    rng, n, a, b, na, nb = fuzz_columns(seed)
    # the condition on the inputs, from the definition alone, before anything runs on the device
    c = [cmp(x, y) for x, y in zip(a, b) if x is not None and y is not None]
    for v in (-1, 0, 1):
        assert c.count(v) >= 0.10 * len(c), (seed, v, c.count(v), len(c))
    x = rng.integers(-5, 6, n).astype(np.int64)
    p = build(oracle, dfdb_mod, {"a": S(a, na), "b": S(b, nb), "x": x}, block_size=1000)
    op = list(OPS)[int(rng.integers(0, 6))]
    l, r = (0, 1) if rng.random() < 0.5 else (1, 0)
    e = IR_OPS[op](ir.col(l), ir.col(r))
    pred = ir.coalesce(e, False) if (na or nb) else e
    others = []
    bound = n
    for _ in range(int(rng.integers(0, 3))):                                          # the kinds of stage test_gpu_fuzz.py draws
        k = rng.random()
        if k < 0.5 or bound < 2:
            others.append(("pred", [ir.col(2) > int(rng.integers(-4, 4)), (ir.col(2) % 3 == 0) | (ir.col(2) > 2), ir.col(2) * 2 != 4][int(rng.integers(0, 3))]))
        elif k < 0.8:
            lo = int(rng.integers(1, bound // 2 + 1)); hi = int(rng.integers(lo, bound + 1)); step = int([1, 2, 3, 64][int(rng.integers(0, 4))])
            others.append(("range", lo, step, hi)); bound = len(range(lo, hi + 1, step))
        else:
            idx = [int(v) for v in rng.integers(1, bound + 1, int(rng.integers(0, 40)))]
            others.append(("idx", idx)); bound = len(set(idx))
    pos = int(rng.integers(0, len(others) + 1))
    stages = others[:pos] + [("pred", pred)] + others[pos:]
    proj = [None, [("x", ir.col(2)), ("a", ir.col(0))], [("r", e), ("b", ir.col(1))]][int(rng.integers(0, 3))]
    check(ctx, p, stages, proj=proj, kern=kern, only_kernel=False)
    p.d.close()
