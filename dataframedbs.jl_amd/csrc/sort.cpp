// sort.cpp — ordering on the device: dfdb_sort_indices (the stable sortperm of the selected rows by one projection column, with a limit), dfdb_sort_indices_n
// (the same by several columns, the most minor key first), dfdb_sort_indices_any (the same with String keys admitted: a String key is m + 1 eight-byte
// sub-keys of the same driver) and dfdb_gather_rows (the projection at given rows, in the given order), over the kernels of k_sort.hip;
// dfdb_gather_rows_any and dfdb_gather_rows_string_bytes (the same gather with String columns admitted), over those of k_str_rows.hip.  ONE sort driver
// (query_sort_indices_n: a single key is its n = 1 case) and ONE gather driver (query_gather_rows) stand behind them.
//
// Replaces sortperm(collect(col)), partialsortperm and sort over Base.iterate(::DFColumn) (src/tables/column.jl:102-126), which pull every selected value to
// the host.  The host side here plans: which rows are kept (the top-k cut, found with the radix select of k_select.hip), which key bytes order anything (the
// per-byte histograms the build leaves), and where the missing rows go; every row and every key stays on the device.
#include "engine.hpp"
#include "ooc.hpp"
#include "select_key.hpp"
#include <algorithm>

namespace dfdb {

// the plain fixed-width projection column p of q, resident and decoded — or the refusal that names the form (`what`: "sorting by" / "gathering rows of").
// strings: a plain String column is admitted too (its flat form: sizes, arena, tile offsets — a column with a dictionary keeps it) when its tiles are short enough
const Column& ordered_column(dfdb_query* q, int32_t p, const char* what, bool strings) {
  if (p < 0 || (size_t)p >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", p);
  const Node& e = *q->proj[(size_t)p].expr;
  const bool str = dt_base(e.dtype) == DFDB_STRING;
  if (str && !strings) fail(DFDB_ERR_UNSUPPORTED, "%s a String column is not supported", what);
  if (e.op != DFIR_COL) fail(DFDB_ERR_UNSUPPORTED, "%s a computed column is not supported: materialise it as a column first (dfdb_table_add_from_query)", what);
  if (!str && !dt_isnum(e.dtype)) fail(DFDB_ERR_UNSUPPORTED, "%s a column of %s is not supported", what, dt_name(e.dtype).c_str());
  dfdb_table* t = q->t;
  if (query_out_of_core(q)) fail(DFDB_ERR_UNSUPPORTED, "%s a column of a view that is out of core (its columns are not resident) is not supported: dfdb_table_load the columns first", what);
  if (t->cols[(size_t)e.col].comp_only)
    fail(DFDB_ERR_UNSUPPORTED, "%s the compressed-only column %s (keep_compressed = 2) is not supported: dfdb_table_decode_resident it first", what, t->cols[(size_t)e.col].name.c_str());
  const Column& col = need_resident(t, e.col);
  if (str && col.max_tile_bytes >= kStrGatherMaxTileBytes)
    fail(DFDB_ERR_UNSUPPORTED, "%s the String column %s is not supported: a 1024-row tile of it holds %u bytes, the limit is below %u (1024 outputs may repeat its longest row, and "
         "their byte total is kept in 32 bits)", what, col.name.c_str(), col.max_tile_bytes, kStrGatherMaxTileBytes);
  return col;
}

namespace {
// the sort's device memory: taken from the pool, back to it when the call ends (the stream drained first)
struct SortScratch {
  dfdb_ctx* ctx;
  DevBuf keys[2], rows[2], miss_rows, order, tile_cnt, tile_base, scan_scratch, counts, starts, hist, stage, row_off;     // row_off: a String key's in-tile offsets
  explicit SortScratch(dfdb_ctx* c) : ctx(c) {}
  ~SortScratch() {
    (void)hipStreamSynchronize(ctx->stream);
    RecycleScope rs;
    for (DevBuf* b : {&keys[0], &keys[1], &rows[0], &rows[1], &miss_rows, &order, &tile_cnt, &tile_base, &scan_scratch, &counts, &starts, &hist, &stage, &row_off}) b->release();
  }
};
struct SortPlan { int64_t nlive = 0, nmiss = 0, L = 0; bool cut = false; uint64_t cutkey = 0; };
}  // namespace

// How many of the first `limit` results are live (L), and — when 0 < L < nlive — the select key of rank L in the sort direction, by the radix select of
// dfdb_order_statistics.  A nullable column's first pass counts its live and missing selected rows (the rank is only known after it); a column without
// a missing bitmap has nlive = sel and takes no pass unless there is a cut to find.
static SortPlan plan_sort(dfdb_query* q, const Column& col, bool rev, int64_t limit, int64_t sel) {
  SortPlan P;
  int64_t cnt[3] = {sel, 0, 0};
  select_keys(q, col, false, dt_nullable(col.dtype), 1, cnt, [&](SelectRanks& R) {
    P.nlive = cnt[0]; P.nmiss = cnt[1];
    P.L = limit < 0 ? P.nlive : (rev ? std::max<int64_t>(0, std::min(limit - P.nmiss, P.nlive)) : std::min(limit, P.nlive));
    P.cut = 0 < P.L && P.L < P.nlive;
    if (P.cut) { R.n = 1; R.rank[0] = rev ? P.nlive - P.L + 1 : P.L; }      // the cut key's rank in ascending order
  }, &P.cutkey);
  return P;
}

static uint64_t flip_of(int nbits, bool rev) { return rev ? (nbits == 64 ? ~0ull : (1ull << nbits) - 1ull) : 0ull; }
static void check_sort_flags(int32_t flags) {
  if (flags & ~DFDB_SORT_REV) fail(DFDB_ERR_ARGUMENT, "ArgumentError: sort flags %d (DFDB_SORT_REV is the only one)", flags);
}
static void check_sort_rows(const dfdb_table* t) {
  if (t->nrows >= (int64_t)1 << 31) fail(DFDB_ERR_UNSUPPORTED, "sorting a table of 2^31 rows or more is not supported: the pairs carry rows in 32 bits");
}

// The count phase of a build (Rec: SortBuild) or a rekey (SortRekey) over ntiles tiles: `count` launches the kernel that fills R.live_cnt / R.miss_cnt, both are
// scanned into R.live_base / R.miss_base and their totals read back: {the pairs, the missing rows}
struct SortCounts { int64_t npairs, nmiss; };
template <class Rec, class Count> static SortCounts sort_count_phase(dfdb_ctx* ctx, SortScratch& S, int64_t ntiles, Rec& R, Count&& count) {
  hipStream_t s = ctx->stream;
  S.tile_cnt.ensure((size_t)(ntiles + 8) * 4 * 2); S.tile_base.ensure((size_t)(ntiles + 8) * 8 * 2); S.scan_scratch.ensure(scan_counts_scratch_bytes(ntiles));
  R.live_cnt = S.tile_cnt.as<uint32_t>(); R.miss_cnt = R.live_cnt + (ntiles + 8);
  count();
  uint64_t* lb = S.tile_base.as<uint64_t>(); uint64_t* mb = lb + (ntiles + 8);
  { LaunchTimer lt(ctx, "scan_counts");
    launch_scan_counts(s, R.live_cnt, lb, ntiles, S.scan_scratch.as<uint64_t>());
    launch_scan_counts(s, R.miss_cnt, mb, ntiles, S.scan_scratch.as<uint64_t>()); }
  HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, lb + ntiles, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar + 1, mb + ntiles, 8, hipMemcpyDeviceToHost, s));
  stream_wait(ctx);
  R.live_base = lb; R.miss_base = mb;
  return {ctx->pinned_scalar[0], ctx->pinned_scalar[1]};
}

// The build from the selection: the pairs of the selected rows `col` keeps (not missing; P.cut: key <= the cut; P.L == 0: none) into S.keys[0] / S.rows[0]
// and the selected missing rows into S.miss_rows, both in table order; the kept keys' per-byte histograms into S.hist.  Returns the pairs; *nmiss: the
// missing rows.  check: the counts must agree with the plan's
static int64_t sort_build_pairs(dfdb_query* q, const Column& col, SortScratch& S, bool rev, const SortPlan& P, bool check, int64_t sel, int64_t* nmiss) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const int nbits = select_key_bits(dt_base(col.dtype), false);
  const int64_t ntiles = ceil_div(t->nrows, kTileRows);
  const uint64_t flip = flip_of(nbits, rev);
  SortBuild B{};
  B.bitmap = q->bitmap.as<uint64_t>(); B.tile_counts = q->tile_counts.as<uint32_t>(); B.nrows = t->nrows;
  B.flip = flip; B.cut = P.cutkey ^ flip; B.keep = P.L == 0 ? SORT_KEEP_NONE : (P.cut ? SORT_KEEP_CUT : SORT_KEEP_ALL);
  int64_t npairs = sel;
  *nmiss = 0;
  if (!dt_nullable(col.dtype) && !P.cut) B.live_base = q->prefix.as<uint64_t>();     // every selected row is kept: the selection's own scan places them
  else {                                                                // count the kept and the missing rows per tile, scan both
    const SortCounts c = sort_count_phase(ctx, S, ntiles, B, [&] {
      HIP_CHECK(hipMemsetAsync(B.live_cnt, 0, (size_t)(ntiles + 8) * 4 * 2, s));       // (a tile with no selected row writes no count)
      LaunchTimer lt(ctx, "sort_build"); launch_sort_build(s, col_ref(col), B, true); });
    npairs = c.npairs; *nmiss = c.nmiss;
    if (check && (*nmiss != P.nmiss || npairs < P.L)) fail(DFDB_ERR_DEVICE, "sort: the build counted %lld kept and %lld missing rows, the plan has %lld and %lld",
                                                           (long long)npairs, (long long)*nmiss, (long long)P.L, (long long)P.nmiss);
  }
  S.keys[0].ensure((size_t)std::max<int64_t>(npairs, 1) * 8); S.rows[0].ensure((size_t)std::max<int64_t>(npairs, 1) * 4);
  S.miss_rows.ensure((size_t)std::max<int64_t>(*nmiss, 1) * 4);
  S.hist.ensure((size_t)(kSelectMaxRanks * 256 + 8) * 8);
  B.keys = S.keys[0].as<uint64_t>(); B.rows = S.rows[0].as<uint32_t>(); B.cap = npairs;
  B.miss_rows = S.miss_rows.as<uint32_t>(); B.miss_cap = *nmiss;
  B.ghist = (unsigned long long*)S.hist.p;
  HIP_CHECK(hipMemsetAsync(S.hist.p, 0, (size_t)(nbits / 8) * 256 * 8, s));
  { LaunchTimer lt(ctx, "sort_build"); launch_sort_build(s, col_ref(col), B, false); }
  return npairs;
}

// The passes over the npairs pairs of S.keys[0] / S.rows[0], by the histograms a build left in S.hist: a byte whose histogram has a single non-zero bin
// orders nothing and its pass is not run.  Returns the half that holds the sorted pairs; *run: the passes run.  pair_cap >= npairs: the pairs the second half
// is made for (the most any key of the call has).  tail: the word the build left behind its histograms (a String key's longest live length) is read back
// with them, whatever npairs is
static int sort_run_passes(dfdb_ctx* ctx, SortScratch& S, int64_t npairs, int64_t pair_cap, int nbytes, int64_t* run, uint64_t* tail = nullptr) {
  hipStream_t s = ctx->stream;
  int cur = 0;
  *run = 0;
  if (npairs <= 1 && !tail) return cur;
  std::vector<uint64_t> gh((size_t)nbytes * 256 + (tail ? 1 : 0));
  HIP_CHECK(hipMemcpyAsync(gh.data(), S.hist.p, gh.size() * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));              // (`gh` is pageable host memory)
  if (tail) *tail = gh[(size_t)nbytes * 256];
  if (npairs <= 1) return cur;
  const int64_t nchunks = sort_chunks(npairs), cchunks = sort_chunks(pair_cap);
  for (int b = 0; b < nbytes; b++) {
    int used = 0;
    for (int d = 0; d < 256; d++) used += gh[(size_t)b * 256 + (size_t)d] != 0;
    if (used <= 1) continue;
    if (!S.keys[1].p) {
      S.keys[1].ensure((size_t)pair_cap * 8); S.rows[1].ensure((size_t)pair_cap * 4);
      S.counts.ensure((size_t)(256 * cchunks + 8) * 4); S.starts.ensure((size_t)(256 * cchunks + 8) * 8); S.scan_scratch.ensure(scan_counts_scratch_bytes(256 * cchunks));
    }
    { LaunchTimer lt(ctx, "sort_count"); launch_sort_count(s, S.keys[cur].as<uint64_t>(), npairs, 8 * b, S.counts.as<uint32_t>()); }
    { LaunchTimer lt(ctx, "scan_counts"); launch_scan_counts(s, S.counts.as<uint32_t>(), S.starts.as<uint64_t>(), 256 * nchunks, S.scan_scratch.as<uint64_t>()); }
    { LaunchTimer lt(ctx, "sort_scatter");
      launch_sort_scatter(s, S.keys[cur].as<uint64_t>(), S.rows[cur].as<uint32_t>(), npairs, 8 * b, S.starts.as<uint64_t>(), S.keys[cur ^ 1].as<uint64_t>(),
                          S.rows[cur ^ 1].as<uint32_t>()); }
    cur ^= 1;
    ++*run;
  }
  return cur;
}

// first[0 .. first_n) then second[0 .. second_n) as 1-based table rows into the caller's buffer (first_n + second_n = m entries, host or device memory)
static void sort_emit_rows(dfdb_table* t, SortScratch& S, const uint32_t* first, int64_t first_n, const uint32_t* second, int64_t second_n, int64_t* out, int32_t memkind) {
  dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const int64_t m = first_n + second_n;
  int64_t* dst = out;
  if (memkind != DFDB_MEM_DEVICE && m > 0) { S.stage.ensure((size_t)m * 8); dst = S.stage.as<int64_t>(); }
  { LaunchTimer lt(ctx, "sort_emit");
    launch_sort_emit(s, first, first_n, dst, t->row_base);
    launch_sort_emit(s, second, second_n, dst + first_n, t->row_base); }
  if (memkind != DFDB_MEM_DEVICE && m > 0) { HIP_CHECK(hipMemcpyAsync(out, dst, (size_t)m * 8, hipMemcpyDeviceToHost, s)); stream_wait(ctx); }
}

// THE sort driver, the keys taken least significant first: the most minor key is built from the selection; every further key towards the major one is built
// from the ORDER the keys behind it left (k_sort_rekey) and sorted by the same stable passes, so rows equal in it keep that order.  After each key its sorted
// live rows and its missing rows (behind them, REV: before them) are laid into S.order — the next key's input; the last key's two lists are the answer.
// A single key is the n = 1 case, different in its plan alone: its build keeps no more than the limit needs (plan_sort's top-k cut) and its scratch is sized
// by what is kept, where several keys sort every selected row and the limit only cuts what comes back.
// strings (dfdb_sort_indices_any): a key may be a plain String column.  It IS m + 1 keys of this driver — (chunk_0, .., chunk_{m-1}, length), 8 key bytes each,
// the length first (k_sort_strkey) — over row_off built once for the key; m is known when the length has been keyed.  A call with a String key takes the
// several-keys plan whatever nkeys is, and a String key that is the most minor one starts from the selected rows laid ascending into S.order.
// sink (the join on several keys): nothing is emitted; the last key's two lists are laid into one order of ALL selected rows, which leaves with the sink
// together with every String key's m and its column's in-tile offsets.  Such a call takes the several-keys plan too (no cut); what the public entry points answer does not pass through it
void query_sort_indices_n(dfdb_query* q, const int32_t* proj_cols, const int32_t* flags, int32_t nkeys, int64_t limit, int64_t* out, int64_t cap, int32_t memkind,
                          int64_t* n, int64_t* info, bool strings, SortOrderSink* sink) {
  if (nkeys < 1 || nkeys > DFDB_SORT_MAX_KEYS) fail(DFDB_ERR_ARGUMENT, "ArgumentError: %d sort keys (1 to %d)", nkeys, (int)DFDB_SORT_MAX_KEYS);
  if (!proj_cols || !flags) fail(DFDB_ERR_ARGUMENT, "ArgumentError: no sort %s", proj_cols ? "flags" : "columns");
  for (int32_t j = 0; j < nkeys; j++) check_sort_flags(flags[j]);
  const Column* cols[DFDB_SORT_MAX_KEYS];
  bool any_str = false;
  for (int32_t j = 0; j < nkeys; j++) { cols[j] = &ordered_column(q, proj_cols[j], "sorting by", strings); any_str = any_str || dt_base(cols[j]->dtype) == DFDB_STRING; }
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  check_sort_rows(t);
  ensure_executed_checked(q);
  const int64_t sel = query_count(q, -1);
  const int64_t total = limit < 0 ? sel : std::min(limit, sel);
  int64_t inf[4] = {sel, 0, 0, 0};
  for (int32_t j = 0; j < nkeys; j++) inf[3] += dt_base(cols[j]->dtype) == DFDB_STRING ? 8 : select_key_bits(dt_base(cols[j]->dtype), false) / 8;   // (a String key: its length; its chunks when they are known)
  if (n) *n = total;
  const int64_t m = std::min(total, std::max<int64_t>(cap, 0));
  if (m > 0 && !out) fail(DFDB_ERR_ARGUMENT, "ArgumentError: no output buffer");
  // nothing to do: one key with nothing to return (limit = 0 too: the cut would keep no pair); several keys sort whatever the limit is and report that sort
  // in info, so only an empty selection ends them here
  const bool one = nkeys == 1 && !any_str && !sink;
  if (sink) { sink->n = 0; sink->passes = 0; for (int32_t j = 0; j < nkeys; j++) sink->str_chunks[j] = 0; }
  if (one ? total == 0 : sel == 0) { if (info) memcpy(info, inf, sizeof inf); return; }

  SortScratch S(ctx);
  if (!one) { S.keys[0].ensure((size_t)sel * 8); S.rows[0].ensure((size_t)sel * 4); S.miss_rows.ensure((size_t)sel * 4); S.order.ensure((size_t)sel * 4); }
  const int64_t otiles = ceil_div(sel, kTileRows);
  const uint32_t *first = nullptr, *second = nullptr;      // the key's two lists in output order, first_len rows in the first
  int64_t first_len = 0;
  // lay the key behind into the order the next one starts from
  auto lay_order = [&] {
    uint32_t* order = S.order.as<uint32_t>();
    LaunchTimer lt(ctx, "sort_order");
    if (first_len > 0) HIP_CHECK(hipMemcpyAsync(order, first, (size_t)first_len * 4, hipMemcpyDeviceToDevice, s));
    if (sel > first_len) HIP_CHECK(hipMemcpyAsync(order + first_len, second, (size_t)(sel - first_len) * 4, hipMemcpyDeviceToDevice, s));
    return order;
  };
  // the sorted pairs of half `cur` and the missing rows are the key's two lists
  auto key_done = [&](int cur, bool rev, int64_t npairs, int64_t nmiss, int64_t run) {
    inf[1] += npairs; inf[2] += run; inf[3] -= run;
    const uint32_t* live_rows = S.rows[cur].as<uint32_t>();
    first = rev ? S.miss_rows.as<uint32_t>() : live_rows; second = rev ? live_rows : S.miss_rows.as<uint32_t>();
    first_len = rev ? nmiss : npairs;
  };
  for (int32_t j = nkeys - 1; j >= 0; j--) {
    const Column& col = *cols[j];
    const bool rev = (flags[j] & DFDB_SORT_REV) != 0;
    if (dt_base(col.dtype) == DFDB_STRING) {
      S.row_off.ensure((size_t)std::max<int64_t>(t->nrows, 1) * 4);
      { LaunchTimer lt(ctx, "str_row_offsets"); launch_str_row_offsets(s, col.data.as<int32_t>(), S.row_off.as<uint32_t>(), t->nrows); }
      S.hist.ensure((size_t)(kSelectMaxRanks * 256 + 8) * 8);
      uint64_t* max_len = S.hist.as<uint64_t>() + 8 * 256;      // the word behind the eight histograms: read back with them
      int64_t nchunks = 0;                                        // m: known after the length
      for (int64_t k = 0; k <= nchunks; k++) {                  // the length, then chunk m - 1 .. chunk 0: the most minor sub-key first
        const int64_t c = k == 0 ? -1 : nchunks - k;
        uint32_t* order = S.order.as<uint32_t>();
        if (j == nkeys - 1 && c == -1) {                          // no order yet: the selected rows, ascending
          LaunchTimer lt(ctx, "sort_rows");
          launch_sort_rows(s, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), q->prefix.as<uint64_t>(), t->nrows, order, sel);
        } else order = lay_order();
        SortStrKey R{};
        R.order = order; R.n = sel; R.nrows = t->nrows; R.flip = flip_of(64, rev); R.chunk = (int32_t)c;
        int64_t npairs = sel, nmiss = 0;
        if (dt_nullable(col.dtype)) {                             // count the live and the missing entries per 1024 entries of the order, scan both
          const SortCounts cn = sort_count_phase(ctx, S, otiles, R, [&] { LaunchTimer lt(ctx, "sort_strkey"); launch_sort_strkey(s, str_side(col), S.row_off.as<uint32_t>(), R, true); });
          npairs = cn.npairs; nmiss = cn.nmiss;
          if (npairs + nmiss != sel) fail(DFDB_ERR_DEVICE, "sort: the String key counted %lld live and %lld missing rows of %lld", (long long)npairs, (long long)nmiss, (long long)sel);
        }
        R.keys = S.keys[0].as<uint64_t>(); R.rows = S.rows[0].as<uint32_t>(); R.cap = npairs;
        R.miss_rows = S.miss_rows.as<uint32_t>(); R.miss_cap = nmiss;
        R.ghist = (unsigned long long*)S.hist.p;
        R.max_len = c == -1 ? (uint32_t*)max_len : nullptr;
        HIP_CHECK(hipMemsetAsync(S.hist.p, 0, (size_t)(8 * 256 + 1) * 8, s));
        { LaunchTimer lt(ctx, c == -1 ? "sort_strkey_len" : "sort_strkey"); launch_sort_strkey(s, str_side(col), S.row_off.as<uint32_t>(), R, false); }   // (the length's launch loads no offset and no arena byte: timed apart)
        int64_t run = 0;
        uint64_t longest = 0;
        const int cur = sort_run_passes(ctx, S, npairs, sel, 8, &run, c == -1 ? &longest : nullptr);
        key_done(cur, rev, npairs, nmiss, run);
        if (c == -1) {
          if (longest > (uint64_t)DFDB_SORT_MAX_STRING_BYTES)
            fail(DFDB_ERR_UNSUPPORTED, "sorting by the String column %s is not supported: a selected row of it holds %llu bytes, the limit is %d (DFDB_SORT_MAX_STRING_BYTES)",
                 col.name.c_str(), (unsigned long long)longest, (int)DFDB_SORT_MAX_STRING_BYTES);
          nchunks = (int64_t)(longest + 7) / 8;
          inf[3] += 8 * nchunks;
          if (sink) sink->str_chunks[j] = (int32_t)nchunks;
        }
      }
      if (sink) sink->row_off[j] = std::move(S.row_off);      // the key's in-tile offsets leave with the sink (the next String key builds its own)
      continue;
    }
    const int nbits = select_key_bits(dt_base(col.dtype), false), nbytes = nbits / 8;
    int64_t npairs = sel, nmiss = 0;
    if (j == nkeys - 1) {
      SortPlan P; P.L = sel;                                // several keys: no cut, every selected row that is not missing is kept
      if (one) P = plan_sort(q, col, rev, limit, sel);
      npairs = sort_build_pairs(q, col, S, rev, P, one, sel, &nmiss);       // (one key: sized by the pairs kept)
    } else {
      SortRekey R{};
      R.order = lay_order(); R.n = sel; R.nrows = t->nrows; R.flip = flip_of(nbits, rev);
      if (dt_nullable(col.dtype)) {                         // count the live and the missing entries per 1024 entries of the order, scan both
        const SortCounts c = sort_count_phase(ctx, S, otiles, R, [&] { LaunchTimer lt(ctx, "sort_rekey"); launch_sort_rekey(s, col_ref(col), R, true); });
        npairs = c.npairs; nmiss = c.nmiss;
        if (npairs + nmiss != sel) fail(DFDB_ERR_DEVICE, "sort: the rekey counted %lld live and %lld missing rows of %lld", (long long)npairs, (long long)nmiss, (long long)sel);
      }
      R.keys = S.keys[0].as<uint64_t>(); R.rows = S.rows[0].as<uint32_t>(); R.cap = npairs;
      R.miss_rows = S.miss_rows.as<uint32_t>(); R.miss_cap = nmiss;
      R.ghist = (unsigned long long*)S.hist.p;
      HIP_CHECK(hipMemsetAsync(S.hist.p, 0, (size_t)nbytes * 256 * 8, s));
      { LaunchTimer lt(ctx, "sort_rekey"); launch_sort_rekey(s, col_ref(col), R, false); }
    }
    int64_t run = 0;
    const int cur = sort_run_passes(ctx, S, npairs, one ? npairs : sel, nbytes, &run);
    key_done(cur, rev, npairs, nmiss, run);
  }
  if (sink) {                                               // the order of every selected row, handed out instead of emitted
    lay_order();
    sink->order = std::move(S.order); sink->n = sel; sink->passes = inf[2];
    if (info) memcpy(info, inf, sizeof inf);
    return;
  }
  // the first m of the two lists (a cut keeps every pair up to the cut key: no fewer than the limit takes of the live rows)
  const int64_t first_n = std::min(m, first_len);
  sort_emit_rows(t, S, first, first_n, second, m - first_n, out, memkind);
  if (info) memcpy(info, inf, sizeof inf);
}

void query_sort_indices(dfdb_query* q, int32_t p, int32_t flags, int64_t limit, int64_t* out, int64_t cap, int32_t memkind, int64_t* n, int64_t* info) {
  query_sort_indices_n(q, &p, &flags, 1, limit, out, cap, memkind, n, info, false, nullptr);
}

// The sorted pairs of the selected rows of q that are not missing in `col` — ascending, no cut, no limit: the build and the passes of the driver above,
// without its plan and its emit — handed to the caller: `keys` / `rows` receive the half that won (npairs entries; equal keys in ascending row order, the sort
// being stable), *nmiss the selected missing rows (they are not keyed), *passes the digit passes run.  col: a column of q's table that the caller has checked
// (ordered_column; a table below 2^31 rows).  Everything else of the sort goes back to the pool here, the stream drained first; the selection is left as it was found
void query_sorted_key_pairs(dfdb_query* q, const Column& col, DevBuf& keys, DevBuf& rows, int64_t* npairs, int64_t* nmiss, int64_t* passes) {
  ensure_executed_checked(q);
  const int64_t sel = query_count(q, -1);
  *npairs = 0; *nmiss = 0; *passes = 0;
  if (sel == 0) return;
  SortScratch S(q->t->ctx);
  SortPlan P; P.L = sel;                                    // no cut: every selected row that is not missing is kept
  *npairs = sort_build_pairs(q, col, S, false, P, false, sel, nmiss);
  const int cur = sort_run_passes(q->t->ctx, S, *npairs, *npairs, select_key_bits(dt_base(col.dtype), false) / 8, passes);
  keys = std::move(S.keys[cur]); rows = std::move(S.rows[cur]);
}

// ---- the projection at given rows: a fixed-width column by one kernel; a String column (k_str_rows.hip) by the offsets of the gathered sizes, then the bytes -------
namespace {
// A gather's device memory — the rows, the flag word a row outside raises, the String passes' arrays, the staging of host outputs: from the pool, back to it
// when the call ends, the stream drained first.  A call that ends with a wait of its own makes it through wait(), and the destructor does not wait again
struct RowsScratch {
  dfdb_ctx* ctx;
  DevBuf rows, flag, row_off, src_off, grp_bytes, out_off, scan_scratch;
  std::vector<DevBuf> stages;                       // per column: data (a String column: sizes), missing bytes (a String column: bytes)
  const int64_t* drows;                             // r[0 .. n) in device memory: the caller's own, or the copy of a host list in `rows`
  bool drained = false;
  RowsScratch(dfdb_ctx* c, int32_t ncols, const int64_t* r, int64_t n, int32_t rows_memkind) : ctx(c), stages((size_t)ncols * 2), drows(r) {
    if (rows_memkind != DFDB_MEM_DEVICE) {
      rows.ensure((size_t)n * 8); drows = rows.as<int64_t>();
      HIP_CHECK(hipMemcpyAsync(rows.p, r, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    flag.ensure(64);
    HIP_CHECK(hipMemsetAsync(flag.p, 0, 8, ctx->stream));
  }
  void wait() { stream_wait(ctx); drained = true; }
  ~RowsScratch() {
    if (!drained) (void)hipStreamSynchronize(ctx->stream);
    RecycleScope rs;
    for (DevBuf* b : {&rows, &flag, &row_off, &src_off, &grp_bytes, &out_off, &scan_scratch}) b->release();
    for (DevBuf& b : stages) b.release();
  }
};
}  // namespace
[[noreturn]] static void fail_row_outside(const dfdb_table* t) { fail(DFDB_ERR_BOUNDS, "BoundsError: a row outside 1..%lld", (long long)(t->row_base + t->nrows)); }

// fixed-width column `col` at drows[0 .. n) into o (device output: in place; host output: through stage / mstage, queued, not waited for)
static void gather_fixed_column(dfdb_table* t, const Column& col, dfdb_outcol& o, const int64_t* drows, int64_t n, uint32_t* flag, DevBuf& stage, DevBuf& mstage) {
  dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const bool dev = o.memkind == DFDB_MEM_DEVICE, want_missing = dt_nullable(col.dtype) && o.missing;
  const int w = dt_width(col.dtype);
  void* dst = o.data; uint8_t* md = want_missing ? o.missing : nullptr;
  if (!dev) {
    stage.ensure((size_t)n * w); dst = stage.p;
    HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)n * w, s));           // (a refused row writes nothing: the host copy must not carry pool bytes)
    if (want_missing) { mstage.ensure((size_t)n); md = mstage.as<uint8_t>(); HIP_CHECK(hipMemsetAsync(md, 0, (size_t)n, s)); }
  }
  { LaunchTimer lt(ctx, "gather_rows");
    launch_gather_rows(s, drows, n, col.data.p, w, dst, dt_nullable(col.dtype) ? col.missing.as<uint64_t>() : nullptr, md, t->row_base, t->nrows, flag); }
  if (!dev) {
    HIP_CHECK(hipMemcpyAsync(o.data, dst, (size_t)n * w, hipMemcpyDeviceToHost, s));
    if (want_missing) HIP_CHECK(hipMemcpyAsync(o.missing, md, (size_t)n, hipMemcpyDeviceToHost, s));
  }
}

// The sizes pass and the scan of String column `col` at S.drows[0 .. n): S.out_off[groups + 1], and the bytes the rows need (the scan's last entry) — read back
// together with the flag word, whose refusal comes first.  form LAYOUT: totals only; else out_sizes (device memory, n entries) and S.src_off are written too
static int64_t rows_string_layout(dfdb_table* t, const Column& col, RowsScratch& S, int64_t n, StrGatherForm form, int32_t* out_sizes) {
  dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const int64_t ngroups = ceil_div(n, kTileRows);
  S.grp_bytes.ensure((size_t)(ngroups + 8) * 4); S.out_off.ensure((size_t)(ngroups + 8) * 8); S.scan_scratch.ensure(scan_counts_scratch_bytes(ngroups));
  if (form != STR_GATHER_LAYOUT) S.src_off.ensure((size_t)n * 8);
  if (form == STR_GATHER_OFFSETS) {
    S.row_off.ensure((size_t)std::max<int64_t>(t->nrows, 1) * 4);
    LaunchTimer lt(ctx, "str_row_offsets"); launch_str_row_offsets(s, col.data.as<int32_t>(), S.row_off.as<uint32_t>(), t->nrows);
  }
  const StrRows R{S.drows, n, str_side(col), t->row_base, t->nrows, S.flag.as<uint32_t>()};
  { LaunchTimer lt(ctx, "str_rows_sizes"); launch_str_rows_sizes(s, R, form, S.row_off.as<uint32_t>(), out_sizes, S.src_off.as<int64_t>(), S.grp_bytes.as<uint32_t>()); }
  { LaunchTimer lt(ctx, "scan_counts"); launch_scan_counts(s, S.grp_bytes.as<uint32_t>(), S.out_off.as<uint64_t>(), ngroups, S.scan_scratch.as<uint64_t>()); }
  HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, S.flag.p, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar + 1, S.out_off.as<uint64_t>() + ngroups, 8, hipMemcpyDeviceToHost, s));
  stream_wait(ctx);
  if (ctx->pinned_scalar[0] != 0) fail_row_outside(t);
  return ctx->pinned_scalar[1];
}

// String column `col` at S.drows[0 .. n) into o, the view's output p (device output: in place; host output: through the column's two stages, queued, not waited for)
static void gather_string_column(dfdb_table* t, const Column& col, dfdb_outcol& o, int32_t p, RowsScratch& S, int64_t n) {
  dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  DevBuf& stage0 = S.stages[(size_t)p * 2]; DevBuf& stage1 = S.stages[(size_t)p * 2 + 1];
  const StrGatherForm form = str_gather_form(n, t->nrows, ctx_option(ctx, "str_gather_form", 0));
  const bool dev = o.memkind == DFDB_MEM_DEVICE;
  int32_t* sizes = (int32_t*)o.data;
  if (!dev) {
    stage0.ensure((size_t)n * 4); sizes = stage0.as<int32_t>();
    HIP_CHECK(hipMemsetAsync(sizes, 0, (size_t)n * 4, s));           // (a refused row writes nothing: the host copy must not carry pool bytes)
  }
  // the rows' sizes and where their bytes start, then — on the host, before a byte moves — whether the bytes fit
  const int64_t total = rows_string_layout(t, col, S, n, form, sizes);
  const int64_t cap = o.bytes ? o.bytes_cap : 0;
  if (total > cap) fail(DFDB_ERR_BOUNDS, "BoundsError: output column %d needs %lld string bytes, capacity is %lld", p, (long long)total, (long long)cap);
  uint8_t* bytes = o.bytes;
  if (!dev && total > 0) { stage1.ensure((size_t)total + 64); bytes = stage1.as<uint8_t>(); }
  prof_note(ctx, form == STR_GATHER_DIRECT ? "str_rows_sizes.direct" : "str_rows_sizes.offsets");
  if (total > 0) { LaunchTimer lt(ctx, "str_rows_bytes"); launch_str_rows_bytes(s, sizes, S.src_off.as<int64_t>(), n, col.bytes.as<uint8_t>(), S.out_off.as<uint64_t>(), bytes, total); }
  if (!dev) {
    HIP_CHECK(hipMemcpyAsync(o.data, sizes, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (total > 0) HIP_CHECK(hipMemcpyAsync(o.bytes, bytes, (size_t)total, hipMemcpyDeviceToHost, s));
  }
  o.nbytes = total;
}

int64_t query_gather_rows_string_bytes(dfdb_query* q, int32_t i, const int64_t* rows, int64_t n, int32_t rows_memkind) {
  if (n < 0) fail(DFDB_ERR_ARGUMENT, "ArgumentError: %lld rows", (long long)n);
  const Column& col = ordered_column(q, i, "gathering rows of", true);
  if (dt_base(col.dtype) != DFDB_STRING || n == 0) return 0;
  RowsScratch S(q->t->ctx, 0, rows, n, rows_memkind);
  return rows_string_layout(q->t, col, S, n, STR_GATHER_LAYOUT, nullptr);
}

// THE gather driver.  strings: String columns are admitted (dfdb_gather_rows_any); else one is refused by name (dfdb_gather_rows)
void query_gather_rows(dfdb_query* q, const int64_t* rows, int64_t n, int32_t rows_memkind, dfdb_outcol* outs, int32_t ncols, bool strings) {
  if (ncols != (int32_t)q->proj.size()) fail(DFDB_ERR_ARGUMENT, "ArgumentError: view has %zu columns, %d outputs given", q->proj.size(), ncols);
  if (n < 0) fail(DFDB_ERR_ARGUMENT, "ArgumentError: %lld rows", (long long)n);
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx;
  std::vector<const Column*> cols;
  for (int32_t p = 0; p < ncols; p++) cols.push_back(&ordered_column(q, p, "gathering rows of", strings));
  for (int32_t p = 0; p < ncols; p++) {
    outs[p].dtype = q->proj[(size_t)p].expr->dtype; outs[p].count = n; outs[p].nbytes = 0;
    if (n > 0 && !outs[p].data) fail(DFDB_ERR_ARGUMENT, "output column %d has no data buffer", p);
  }
  if (n == 0) return;
  RowsScratch S(ctx, ncols, rows, n, rows_memkind);
  for (int32_t p = 0; p < ncols; p++) {
    const Column& col = *cols[(size_t)p];
    if (dt_base(col.dtype) == DFDB_STRING) gather_string_column(t, col, outs[p], p, S, n);
    else gather_fixed_column(t, col, outs[p], S.drows, n, S.flag.as<uint32_t>(), S.stages[(size_t)p * 2], S.stages[(size_t)p * 2 + 1]);
  }
  HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, S.flag.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  S.wait();                                          // (also: the staging buffers and a pageable `rows` die with this call)
  if (ctx->pinned_scalar[0] != 0) fail_row_outside(t);
}

}  // namespace dfdb
