"""Which launches answer a predicate stage (csrc/query.cpp: plan_predicate / run_plan), pinned per kind of conjunct: every case below is compared with the
oracle through helpers (count, bitmap, indices, materialized columns bit for bit; aggregates against the oracle's materialized values) and its launches are
counted by profile name.  EXPECTED holds those counts as literals, recorded once from the engine as it stood BEFORE the predicate stage was split into a
plan and its run: a case whose route changes — another kernel, one launch more, a capture or an aggregate rider lost or gained — fails here.

Every count covers the whole of helpers.assert_same: one execution for the count (no hint), then materialize's own (dfdb_query_hint_materialize on), so a
predicate-side entry is normally twice its launches per execution and the projection-side entries (gather, compact_captured, str_*) are one materialize.

Sizes: one partial 1024-row tile, exactly one tile, a tile and a row, two tiles and a part.  Not coverable at these sizes: the placement calibration (2^26
rows: test_gpu_context.py) and query_count's retry after a bad decode (test_gpu_compressed.py, test_gpu_compressed_only.py)."""
import numpy as np
import pytest

from helpers import apply_stages, assert_same

pytestmark = pytest.mark.gpu

SIZES = (1, 1024, 1025, 2500)
# every profile entry a predicate stage can launch under, then what the projection side shows of the plan's capture / aggregate / constant decisions
PRED_NAMES = ("interp_predicate", "jit_predicate", "dict_scan", "str_match", "str_pair", "dict_pair", "missing_mask", "scan_cmp", "scan_terms", "scan_terms.pair",
              "lz4_decode_scan_hist")
PROJ_NAMES = ("compact_captured", "gather", "str_compact_captured", "str_gather_bytes", "fill_const_strings", "reduce_partials", "reduce")
NAMES = PRED_NAMES + PROJ_NAMES
WORDS = (b"x", b"y", b"xa", b"zb", b"q", b"xylophone")


class Tab:
    """one table held twice (oracle + engine), as helpers.Pair holds it: two Int64, one UInt64, one Float64, one nullable Int64, two String, one nullable String"""

    def __init__(self, O, dfdb, n, dictionaries=(), block_size=65536, compressed_only=()):
        """dictionaries / compressed_only: names of the String columns that get a dictionary / of the fixed-width columns that keep their LZ4 blocks only"""
        from dfdb import ir
        rng = np.random.default_rng(1000 + n)
        pick = lambda: [WORDS[int(k)] for k in rng.integers(0, len(WORDS), n)]
        ns = pick()
        for r in range(0, n, 7):
            ns[r] = None
        if n == 1:
            ns[0] = b"x"
        self.cols = {
            "a": rng.integers(0, 100, n).astype(np.int64),
            "b": rng.integers(0, 1000, n).astype(np.int64),
            "u": rng.integers(0, 2**63, n).astype(np.uint64) * np.uint64(2),
            "x": rng.integers(0, 8000, n).astype(np.float64) / 4.0,            # multiples of 1/4 below 2^11: every sum of them is exact, in any order
            "n": np.ma.masked_array(rng.integers(0, 100, n).astype(np.int64), mask=(np.arange(n) % 5 == 2)),
            "s1": pick(), "s2": pick(), "ns": ns,
        }
        self.O, self.dfdb, self.names, self.nrows = O, dfdb, list(self.cols), n
        self.o = O.Table(block_size=block_size)
        self.d = dfdb.DFTable.new(block_size)
        for k, v in self.cols.items():
            if isinstance(v, np.ma.MaskedArray):
                self.o.add_column(k, np.ascontiguousarray(v.filled(0)), missing=np.ma.getmaskarray(v))
                self.d.add_column(k, v)
            elif isinstance(v, list):
                nullable = k == "ns"
                self.o.add_column(k, O.strings_to_flat(v), dtype=O.NULLABLE if nullable else None)
                self.d.add_column(k, v, dtype=ir.STRING | (ir.NULLABLE if nullable else 0))
            else:
                self.o.add_column(k, v)
                self.d.add_column(k, v)
        for k in dictionaries:
            assert self.d.build_dictionary(k, 4096) == len(set(self.cols[k]))
        for k in compressed_only:
            self.d.compress_column(k, 2)


def exprs():
    from dfdb import ir
    return tuple(ir.col(k) for k in range(8))


def three(A, B, X):
    """the three-term batch of the capture and aggregate cases: terms 0, 1, 2 read a, b, x"""
    return (A > 10) & (B < 900) & (X < 1800.0)


def cases(n):
    """name -> (stages, projection or None, ctx options).  Built per table size: a range stage names n."""
    from dfdb import ir
    A, B, U, X, N, S1, S2, NS = exprs()
    P = lambda e: [("pred", e)]
    six = (A > 5) & (B < 950) & (U >= 2**60) & (A % 7 != 0) & (B % 5 != 1) & (A * 3 + 1 > 20)
    mix = (A + B > 100) & ~ir.startswith(S1, "z") & (S2 != "q") & (S1 != S2) & ~ir.ismissing(N) & ((A > 50) | (B < 500)) & (A > 2) & (X < 1990.0)
    sw = ir.startswith(S1, "x")
    c = {
        # simple terms
        "one_term": (P(A > 50), None, {}),
        "interval": (P((65 > A) & (A > 34)), None, {}),
        "two_terms": (P((A > 20) & (B < 800)), None, {}),
        "seven_terms": (P(six & (X < 1900.0)), None, {}),                        # kMaxTerms = 6: two batches
        "rem": (P(A % 7 == 3), None, {}),
        # disjunctions and masks
        "or": (P((A > 90) | (B < 100)), None, {}),
        "in_set": (P(ir.isin(A, [3, 50, 77])), None, {}),
        "ismissing": (P(ir.ismissing(N)), None, {}),
        "not_ismissing": (P(~ir.ismissing(N)), None, {}),
        # string terms (s1 and s2 carry dictionaries in the second parametrisation)
        "str_eq": (P(S1 == "x"), None, {}),
        "str_startswith": (P(sw), None, {}),
        "str_not_startswith": (P(~sw), None, {}),
        "str_or": (P((S1 == "x") | (S1 == "y")), None, {}),
        "nullable_str_eq": (P(ir.coalesce(NS == "x", False)), None, {}),
        "pair": (P(S1 < S2), None, {}),
        "nullable_pair": (P(ir.coalesce(NS < S2, False)), None, {}),
        "pair_interp": (P(S1 < S2), None, {"str_pair_kernel": 0}),
        "nullable_pair_interp": (P(ir.coalesce(NS < S2, False)), None, {"str_pair_kernel": 0}),
        # generic conjuncts: any number of them is one interpreter launch
        "generic": (P(A + B > 500), None, {}),
        "two_generic": (P((A + B > 500) & (A * B < 40000)), None, {}),
        # every kind in one stage, and as the second of two stages
        "mix": (P(mix), None, {}),
        "mix_after_range": ([("range", 1, 2, n)] + P(mix), None, {}),
        # hint_materialize: the scan keeps projected predicate columns
        "cap_first": (P(three(A, B, X)), [("a", A)], {}),
        "cap_middle": (P(three(A, B, X)), [("b", B)], {}),
        "cap_last": (P(three(A, B, X)), [("x", X)], {}),
        "cap_first_middle": (P(three(A, B, X)), [("a", A), ("b", B)], {}),
        "cap_first_last": (P(three(A, B, X)), [("a", A), ("x", X)], {}),       # the second captured term already sits last
        "cap_middle_last": (P(three(A, B, X)), [("b", B), ("x", X)], {}),
        "cap_last_first": (P(three(A, B, X)), [("x", X), ("a", A)], {}),
        "cap_middle_first": (P(three(A, B, X)), [("b", B), ("a", A)], {}),
        "cap_last_middle": (P(three(A, B, X)), [("x", X), ("b", B)], {}),
        "cap_all_three": (P(three(A, B, X)), [("a", A), ("b", B), ("x", X)], {}),     # two captured, one gathered
        "cap_transform": (P(three(A, B, X)), [("t", A * 3 + 1)], {}),
        "cap_seven_terms": (P(six & (X < 1900.0)), [("a", A), ("x", X)], {}),         # only the last batch (x alone) captures
        "cap_after_range": ([("range", 1, 2, n)] + P(three(A, B, X)), [("a", A), ("x", X)], {}),
        # the String capture: one non-`==` match alone in a single stage keeps the rows; any other conjunct beside it narrows the mask afterwards
        "strcap_alone": (P(sw), [("s1", S1)], {}),
        "strcap_generic": (P(sw & (A + B > 100)), [("s1", S1)], {}),
        "strcap_dict_lut": (P(sw & ~ir.startswith(S2, "z")), [("s1", S1)], {}),     # (a LUT scan only where s2 alone has a dictionary: test_string_capture_beside_a_dictionary_lut_scan)
        "strcap_second_match": (P(sw & (S2 != "q")), [("s1", S1)], {}),
        "strcap_pair": (P(sw & (S1 <= S2)), [("s1", S1)], {}),
        "strcap_missing": (P(sw & ~ir.ismissing(N)), [("s1", S1)], {}),
        "strcap_or": (P(sw & ((A > 50) | (B < 500))), [("s1", S1)], {}),
        "strcap_term": (P(sw & (A > 2)), [("s1", S1)], {}),
        "strcap_after_range": ([("range", 1, 1, n)] + P(sw), [("s1", S1)], {}),
        "str_eq_projected": (P(S1 == "x"), [("s1", S1), ("a", A)], {}),              # every selected row holds "x": fill_const_strings
    }
    return c


CASE_NAMES = tuple(cases(4))
# hint_aggregate: the hinted column's term first (a) and last (x) in the batch; a rem term of the hinted column must not ride
AGG_CASES = {"first": ("three", 0), "last": ("three", 3), "rem": ("rem", 0)}
AGG_OPS = {"sum": 1, "min": 2, "max": 3}


@pytest.fixture(scope="module")
def tables(oracle, dfdb_mod, ctx):
    made = {}

    def get(n, dictionaries):
        if (n, dictionaries) not in made:
            made[(n, dictionaries)] = Tab(oracle, dfdb_mod, n, dictionaries)
        return made[(n, dictionaries)]
    yield get
    for t in made.values():
        t.d.close()


@pytest.fixture
def interp(ctx):
    """the ahead-of-time interpreter answers every generic conjunct"""
    ctx.set_option("jit", 0)
    yield
    ctx.set_option("jit", 1)


OPTION_DEFAULTS = {"str_pair_kernel": 1}          # what a case may set, and the library's default it goes back to


def counted(ctx, fn, options=None):
    """launches by profile name while fn runs (zero entries left out)"""
    for k, v in (options or {}).items():
        assert k in OPTION_DEFAULTS, k
        ctx.set_option(k, v)
    ctx.profile(True)
    before = [ctx.profile_get(k)[0] for k in NAMES]
    try:
        fn()
        after = [ctx.profile_get(k)[0] for k in NAMES]
    finally:
        ctx.profile(False)
        for k in (options or {}):
            ctx.set_option(k, OPTION_DEFAULTS[k])
    return {k: a - b for k, a, b in zip(NAMES, after, before) if a != b}


def run_case(ctx, tab, name):
    stages, proj, options = cases(tab.nrows)[name]
    ov, dv = apply_stages(tab, stages, proj=proj)
    return counted(ctx, lambda: assert_same(tab, ov, dv), options)


def run_aggregate(ctx, tab, which, op):
    """op over the hinted projection column of a fresh query (the hint goes in before the first execution) against the oracle's selected values"""
    A, B, U, X, N, S1, S2, NS = exprs()
    shape, colord = AGG_CASES[which]
    pred = three(A, B, X) if shape == "three" else (A % 7 == 3) & (B < 900)
    col = exprs()[colord]
    ov, dv = apply_stages(tab, [("pred", pred)], proj=[("v", col)])
    want = ov.materialize()[0]
    got = {}

    def go():
        q = dv._query()
        if len(want) == 0 and op != "sum":
            with pytest.raises(ValueError):
                q.aggregate(AGG_OPS[op], 0)
        else:
            got["v"] = q.aggregate(AGG_OPS[op], 0)
            assert q.count() == len(want)
    n = counted(ctx, go)
    if "v" in got:
        ref = {"sum": np.sum, "min": np.min, "max": np.max}[op](want) if len(want) else 0
        assert got["v"] == ref, (which, op, got["v"], ref)              # exact: integers, and Float64 values whose sums are exact (Tab)
    return n


def expected(table, name, tab, dictionaries):
    e = table[name]["dict" if dictionaries else "plain"]
    return e[tab.nrows] if tab.nrows in e else e


# -------------------------------------------------------------------------------------------------- recorded on the parent commit
EXPECTED = {'one_term': {'plain': {'compact_captured': 1, 'gather': 4, 'scan_cmp': 2, 'str_gather_bytes': 3},
              'dict': {'compact_captured': 1, 'gather': 8, 'scan_cmp': 2, 'str_gather_bytes': 1}},
 'interval': {'plain': {'compact_captured': 1, 'gather': 4, 'scan_terms': 2, 'str_gather_bytes': 3},
              'dict': {'compact_captured': 1, 'gather': 8, 'scan_terms': 2, 'str_gather_bytes': 1}},
 'two_terms': {'plain': {1: {'scan_terms': 2, 'scan_terms.pair': 2},
                         1024: {'compact_captured': 2, 'gather': 3, 'scan_terms': 2, 'scan_terms.pair': 2, 'str_gather_bytes': 3},
                         1025: {'compact_captured': 2, 'gather': 3, 'scan_terms': 2, 'scan_terms.pair': 2, 'str_gather_bytes': 3},
                         2500: {'compact_captured': 2, 'gather': 3, 'scan_terms': 2, 'scan_terms.pair': 2, 'str_gather_bytes': 3}},
               'dict': {1: {'gather': 2, 'scan_terms': 2, 'scan_terms.pair': 2},
                        1024: {'compact_captured': 2, 'gather': 7, 'scan_terms': 2, 'scan_terms.pair': 2, 'str_gather_bytes': 1},
                        1025: {'compact_captured': 2, 'gather': 7, 'scan_terms': 2, 'scan_terms.pair': 2, 'str_gather_bytes': 1},
                        2500: {'compact_captured': 2, 'gather': 7, 'scan_terms': 2, 'scan_terms.pair': 2, 'str_gather_bytes': 1}}},
 'seven_terms': {'plain': {'compact_captured': 1, 'gather': 4, 'scan_cmp': 1, 'scan_terms': 3, 'str_gather_bytes': 3},
                 'dict': {'compact_captured': 1, 'gather': 8, 'scan_cmp': 1, 'scan_terms': 3, 'str_gather_bytes': 1}},
 'rem': {'plain': {1: {'scan_terms': 2},
                   1024: {'gather': 5, 'scan_terms': 2, 'str_gather_bytes': 3},
                   1025: {'gather': 5, 'scan_terms': 2, 'str_gather_bytes': 3},
                   2500: {'gather': 5, 'scan_terms': 2, 'str_gather_bytes': 3}},
         'dict': {1: {'gather': 2, 'scan_terms': 2},
                  1024: {'gather': 9, 'scan_terms': 2, 'str_gather_bytes': 1},
                  1025: {'gather': 9, 'scan_terms': 2, 'str_gather_bytes': 1},
                  2500: {'gather': 9, 'scan_terms': 2, 'str_gather_bytes': 1}}},
 'or': {'plain': {1: {'scan_terms': 2},
                  1024: {'gather': 5, 'scan_terms': 2, 'str_gather_bytes': 3},
                  1025: {'gather': 5, 'scan_terms': 2, 'str_gather_bytes': 3},
                  2500: {'gather': 5, 'scan_terms': 2, 'str_gather_bytes': 3}},
        'dict': {1: {'gather': 2, 'scan_terms': 2},
                 1024: {'gather': 9, 'scan_terms': 2, 'str_gather_bytes': 1},
                 1025: {'gather': 9, 'scan_terms': 2, 'str_gather_bytes': 1},
                 2500: {'gather': 9, 'scan_terms': 2, 'str_gather_bytes': 1}}},
 'in_set': {'plain': {1: {'scan_terms': 2},
                      1024: {'gather': 5, 'scan_terms': 2, 'str_gather_bytes': 3},
                      1025: {'gather': 5, 'scan_terms': 2, 'str_gather_bytes': 3},
                      2500: {'gather': 5, 'scan_terms': 2, 'str_gather_bytes': 3}},
            'dict': {1: {'gather': 2, 'scan_terms': 2},
                     1024: {'gather': 9, 'scan_terms': 2, 'str_gather_bytes': 1},
                     1025: {'gather': 9, 'scan_terms': 2, 'str_gather_bytes': 1},
                     2500: {'gather': 9, 'scan_terms': 2, 'str_gather_bytes': 1}}},
 'ismissing': {'plain': {1: {'missing_mask': 2},
                         1024: {'gather': 5, 'missing_mask': 2, 'str_gather_bytes': 3},
                         1025: {'gather': 5, 'missing_mask': 2, 'str_gather_bytes': 3},
                         2500: {'gather': 5, 'missing_mask': 2, 'str_gather_bytes': 3}},
               'dict': {1: {'gather': 2, 'missing_mask': 2},
                        1024: {'gather': 9, 'missing_mask': 2, 'str_gather_bytes': 1},
                        1025: {'gather': 9, 'missing_mask': 2, 'str_gather_bytes': 1},
                        2500: {'gather': 9, 'missing_mask': 2, 'str_gather_bytes': 1}}},
 'not_ismissing': {'plain': {'gather': 5, 'missing_mask': 2, 'str_gather_bytes': 3}, 'dict': {'gather': 9, 'missing_mask': 2, 'str_gather_bytes': 1}},
 'str_eq': {'plain': {1: {'str_match': 2},
                      1024: {'fill_const_strings': 1, 'gather': 5, 'str_gather_bytes': 2, 'str_match': 2},
                      1025: {'fill_const_strings': 1, 'gather': 5, 'str_gather_bytes': 2, 'str_match': 2},
                      2500: {'fill_const_strings': 1, 'gather': 5, 'str_gather_bytes': 2, 'str_match': 2}},
            'dict': {1: {'dict_scan': 2, 'gather': 1},
                     1024: {'dict_scan': 2, 'fill_const_strings': 1, 'gather': 7, 'str_gather_bytes': 1},
                     1025: {'dict_scan': 2, 'fill_const_strings': 1, 'gather': 7, 'str_gather_bytes': 1},
                     2500: {'dict_scan': 2, 'fill_const_strings': 1, 'gather': 7, 'str_gather_bytes': 1}}},
 'str_startswith': {'plain': {'gather': 5, 'str_compact_captured': 1, 'str_gather_bytes': 2, 'str_match': 2},
                    'dict': {'dict_scan': 2, 'gather': 9, 'str_gather_bytes': 1}},
 'str_not_startswith': {'plain': {1: {'interp_predicate': 2},
                                  1024: {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3},
                                  1025: {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3},
                                  2500: {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3}},
                        'dict': {1: {'dict_scan': 2, 'gather': 2},
                                 1024: {'dict_scan': 2, 'gather': 9, 'str_gather_bytes': 1},
                                 1025: {'dict_scan': 2, 'gather': 9, 'str_gather_bytes': 1},
                                 2500: {'dict_scan': 2, 'gather': 9, 'str_gather_bytes': 1}}},
 'str_or': {'plain': {1: {'interp_predicate': 2},
                      1024: {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3},
                      1025: {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3},
                      2500: {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3}},
            'dict': {1: {'dict_scan': 2, 'gather': 2},
                     1024: {'dict_scan': 2, 'gather': 9, 'str_gather_bytes': 1},
                     1025: {'dict_scan': 2, 'gather': 9, 'str_gather_bytes': 1},
                     2500: {'dict_scan': 2, 'gather': 9, 'str_gather_bytes': 1}}},
 'nullable_str_eq': {'plain': {'gather': 5, 'str_gather_bytes': 3, 'str_match': 2}, 'dict': {'gather': 9, 'str_gather_bytes': 1, 'str_match': 2}},
 'pair': {'plain': {'gather': 5, 'str_gather_bytes': 3, 'str_pair': 2}, 'dict': {'dict_pair': 2, 'gather': 9, 'str_gather_bytes': 1}},
 'nullable_pair': {'plain': {'gather': 5, 'str_gather_bytes': 3, 'str_pair': 2}, 'dict': {'gather': 9, 'str_gather_bytes': 1, 'str_pair': 2}},
 'pair_interp': {'plain': {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3}, 'dict': {'gather': 9, 'interp_predicate': 2, 'str_gather_bytes': 1}},
 'nullable_pair_interp': {'plain': {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3}, 'dict': {'gather': 9, 'interp_predicate': 2, 'str_gather_bytes': 1}},
 'generic': {'plain': {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3}, 'dict': {'gather': 9, 'interp_predicate': 2, 'str_gather_bytes': 1}},
 'two_generic': {'plain': {1: {'interp_predicate': 2},
                           1024: {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3},
                           1025: {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3},
                           2500: {'gather': 5, 'interp_predicate': 2, 'str_gather_bytes': 3}},
                 'dict': {1: {'gather': 2, 'interp_predicate': 2},
                          1024: {'gather': 9, 'interp_predicate': 2, 'str_gather_bytes': 1},
                          1025: {'gather': 9, 'interp_predicate': 2, 'str_gather_bytes': 1},
                          2500: {'gather': 9, 'interp_predicate': 2, 'str_gather_bytes': 1}}},
 'mix': {'plain': {'compact_captured': 2, 'gather': 3, 'interp_predicate': 2, 'missing_mask': 2, 'scan_terms': 4, 'str_gather_bytes': 3, 'str_match': 2, 'str_pair': 2},
         'dict': {'compact_captured': 2, 'dict_pair': 2, 'dict_scan': 4, 'gather': 7, 'interp_predicate': 2, 'missing_mask': 2, 'scan_terms': 4, 'str_gather_bytes': 1}},
 'mix_after_range': {'plain': {'compact_captured': 2,
                               'gather': 3,
                               'interp_predicate': 2,
                               'missing_mask': 2,
                               'scan_terms': 4,
                               'str_gather_bytes': 3,
                               'str_match': 2,
                               'str_pair': 2},
                     'dict': {'compact_captured': 2,
                              'dict_pair': 2,
                              'dict_scan': 4,
                              'gather': 7,
                              'interp_predicate': 2,
                              'missing_mask': 2,
                              'scan_terms': 4,
                              'str_gather_bytes': 1}},
 'cap_first': {'plain': {'compact_captured': 1, 'scan_terms': 2}, 'dict': {'compact_captured': 1, 'scan_terms': 2}},
 'cap_middle': {'plain': {'compact_captured': 1, 'scan_terms': 2}, 'dict': {'compact_captured': 1, 'scan_terms': 2}},
 'cap_last': {'plain': {'compact_captured': 1, 'scan_terms': 2}, 'dict': {'compact_captured': 1, 'scan_terms': 2}},
 'cap_first_middle': {'plain': {'compact_captured': 2, 'scan_terms': 2}, 'dict': {'compact_captured': 2, 'scan_terms': 2}},
 'cap_first_last': {'plain': {'compact_captured': 2, 'scan_terms': 2}, 'dict': {'compact_captured': 2, 'scan_terms': 2}},
 'cap_middle_last': {'plain': {'compact_captured': 2, 'scan_terms': 2}, 'dict': {'compact_captured': 2, 'scan_terms': 2}},
 'cap_last_first': {'plain': {'compact_captured': 2, 'scan_terms': 2}, 'dict': {'compact_captured': 2, 'scan_terms': 2}},
 'cap_middle_first': {'plain': {'compact_captured': 2, 'scan_terms': 2}, 'dict': {'compact_captured': 2, 'scan_terms': 2}},
 'cap_last_middle': {'plain': {'compact_captured': 2, 'scan_terms': 2}, 'dict': {'compact_captured': 2, 'scan_terms': 2}},
 'cap_all_three': {'plain': {'compact_captured': 2, 'gather': 1, 'scan_terms': 2}, 'dict': {'compact_captured': 2, 'gather': 1, 'scan_terms': 2}},
 'cap_transform': {'plain': {'compact_captured': 1, 'scan_terms': 2}, 'dict': {'compact_captured': 1, 'scan_terms': 2}},
 'cap_seven_terms': {'plain': {'compact_captured': 1, 'gather': 1, 'scan_cmp': 1, 'scan_terms': 3},
                     'dict': {'compact_captured': 1, 'gather': 1, 'scan_cmp': 1, 'scan_terms': 3}},
 'cap_after_range': {'plain': {'compact_captured': 2, 'scan_terms': 2}, 'dict': {'compact_captured': 2, 'scan_terms': 2}},
 'strcap_alone': {'plain': {'str_compact_captured': 1, 'str_match': 2}, 'dict': {'dict_scan': 2, 'gather': 2}},
 'strcap_generic': {'plain': {'interp_predicate': 2, 'str_gather_bytes': 1, 'str_match': 2}, 'dict': {'dict_scan': 2, 'gather': 2, 'interp_predicate': 2}},
 'strcap_dict_lut': {'plain': {'interp_predicate': 2, 'str_gather_bytes': 1, 'str_match': 2}, 'dict': {'dict_scan': 4, 'gather': 2}},
 'strcap_second_match': {'plain': {'str_gather_bytes': 1, 'str_match': 4}, 'dict': {'dict_scan': 4, 'gather': 2}},
 'strcap_pair': {'plain': {'str_gather_bytes': 1, 'str_match': 2, 'str_pair': 2}, 'dict': {'dict_pair': 2, 'dict_scan': 2, 'gather': 2}},
 'strcap_missing': {'plain': {'missing_mask': 2, 'str_gather_bytes': 1, 'str_match': 2}, 'dict': {'dict_scan': 2, 'gather': 2, 'missing_mask': 2}},
 'strcap_or': {'plain': {'scan_terms': 2, 'str_gather_bytes': 1, 'str_match': 2}, 'dict': {'dict_scan': 2, 'gather': 2, 'scan_terms': 2}},
 'strcap_term': {'plain': {'scan_cmp': 2, 'str_gather_bytes': 1, 'str_match': 2}, 'dict': {'dict_scan': 2, 'gather': 2, 'scan_cmp': 2}},
 'strcap_after_range': {'plain': {'str_gather_bytes': 1, 'str_match': 2}, 'dict': {'dict_scan': 2, 'gather': 2}},
 'str_eq_projected': {'plain': {1: {'str_match': 2},
                                1024: {'fill_const_strings': 1, 'gather': 1, 'str_match': 2},
                                1025: {'fill_const_strings': 1, 'gather': 1, 'str_match': 2},
                                2500: {'fill_const_strings': 1, 'gather': 1, 'str_match': 2}},
                      'dict': {1: {'dict_scan': 2},
                               1024: {'dict_scan': 2, 'fill_const_strings': 1, 'gather': 1},
                               1025: {'dict_scan': 2, 'fill_const_strings': 1, 'gather': 1},
                               2500: {'dict_scan': 2, 'fill_const_strings': 1, 'gather': 1}}}}
EXPECTED_AGG = {'first_max': {'plain': {'reduce_partials': 1, 'scan_terms': 1}},
 'first_min': {'plain': {'reduce_partials': 1, 'scan_terms': 1}},
 'first_sum': {'plain': {'reduce_partials': 1, 'scan_terms': 1}},
 'last_max': {'plain': {'reduce_partials': 1, 'scan_terms': 1}},
 'last_min': {'plain': {'reduce_partials': 1, 'scan_terms': 1}},
 'last_sum': {'plain': {'reduce_partials': 1, 'scan_terms': 1}},
 'rem_max': {'plain': {'reduce': 1, 'scan_terms': 1}},
 'rem_min': {'plain': {'reduce': 1, 'scan_terms': 1}},
 'rem_sum': {'plain': {'reduce': 1, 'scan_terms': 1}}}
EXPECTED_S2_DICT = {1: {'dict_scan': 2, 'str_gather_bytes': 1, 'str_match': 2},
 1024: {'dict_scan': 2, 'str_gather_bytes': 1, 'str_match': 2},
 1025: {'dict_scan': 2, 'str_gather_bytes': 1, 'str_match': 2},
 2500: {'dict_scan': 2, 'str_gather_bytes': 1, 'str_match': 2}}
EXPECTED_COMP = {1: {'lz4_decode_scan_hist': 2, 'str_gather_bytes': 1, 'str_match': 2},
 1024: {'lz4_decode_scan_hist': 2, 'str_gather_bytes': 1, 'str_match': 2},
 1025: {'lz4_decode_scan_hist': 2, 'str_gather_bytes': 1, 'str_match': 2},
 2500: {'lz4_decode_scan_hist': 2, 'str_gather_bytes': 1, 'str_match': 2}}
# --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("dictionaries", [False, True], ids=["plain", "dict"])
@pytest.mark.parametrize("n", SIZES)
def test_route(ctx, interp, tables, n, dictionaries, name):
    tab = tables(n, ("s1", "s2") if dictionaries else ())
    assert run_case(ctx, tab, name) == expected(EXPECTED, name, tab, dictionaries)


@pytest.mark.parametrize("op", list(AGG_OPS))
@pytest.mark.parametrize("which", list(AGG_CASES))
@pytest.mark.parametrize("n", SIZES)
def test_aggregate_rider(ctx, interp, tables, n, which, op):
    tab = tables(n, ())
    assert run_aggregate(ctx, tab, which, op) == expected(EXPECTED_AGG, which + "_" + op, tab, False)


@pytest.mark.parametrize("n", SIZES)
def test_string_capture_beside_a_dictionary_lut_scan(ctx, interp, tables, n):
    """only s2 carries a dictionary: `!startswith(s2, "z")` is a LUT scan of its codes beside the flat, capturable match on s1 — which must not capture"""
    assert run_case(ctx, tables(n, ("s2",)), "strcap_dict_lut") == EXPECTED_S2_DICT[n]


@pytest.mark.parametrize("n", SIZES)
def test_string_capture_beside_a_compressed_only_scan(oracle, dfdb_mod, ctx, interp, n):
    """the one kind of conjunct the shared tables cannot hold: `b` keeps its LZ4 blocks only, so `b < 900` is the decoder's own scan — and the String
    capture beside it must not happen"""
    from dfdb import ir
    tab = Tab(oracle, dfdb_mod, n, block_size=1024, compressed_only=("b",))
    try:
        A, B, U, X, N, S1, S2, NS = exprs()
        ov, dv = apply_stages(tab, [("pred", ir.startswith(S1, "x") & (B < 900))], proj=[("s1", S1)])
        got = counted(ctx, lambda: assert_same(tab, ov, dv))
    finally:
        tab.d.close()
    assert got == EXPECTED_COMP[n]
