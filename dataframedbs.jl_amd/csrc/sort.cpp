// sort.cpp — ordering on the device: dfdb_sort_indices (the stable sortperm of the selected rows by one projection column, with a limit) and
// dfdb_gather_rows (the projection at given rows, in the given order), over the kernels of k_sort.hip.
//
// Replaces sortperm(collect(col)), partialsortperm and sort over Base.iterate(::DFColumn) (src/tables/column.jl:102-126), which pull every selected value to
// the host.  The host side here plans: which rows are kept (the top-k cut, found with the radix select of k_select.hip), which key bytes order anything (the
// per-byte histograms the build leaves), and where the missing rows go; every row and every key stays on the device.
#include "engine.hpp"
#include "ooc.hpp"
#include "select_key.hpp"
#include <algorithm>

namespace dfdb {

// the plain fixed-width projection column p of q, resident and decoded — or the refusal that names the form (`what`: "sorting by" / "gathering rows of")
static const Column& ordered_column(dfdb_query* q, int32_t p, const char* what) {
  if (p < 0 || (size_t)p >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", p);
  const Node& e = *q->proj[(size_t)p].expr;
  if (dt_base(e.dtype) == DFDB_STRING) fail(DFDB_ERR_UNSUPPORTED, "%s a String column is not supported", what);
  if (e.op != DFIR_COL) fail(DFDB_ERR_UNSUPPORTED, "%s a computed column is not supported: materialise it as a column first (dfdb_table_add_from_query)", what);
  if (!dt_isnum(e.dtype)) fail(DFDB_ERR_UNSUPPORTED, "%s a column of %s is not supported", what, dt_name(e.dtype).c_str());
  dfdb_table* t = q->t;
  if (query_out_of_core(q)) fail(DFDB_ERR_UNSUPPORTED, "%s a column of a view that is out of core (its columns are not resident) is not supported: dfdb_table_load the columns first", what);
  if (t->cols[(size_t)e.col].comp_only)
    fail(DFDB_ERR_UNSUPPORTED, "%s the compressed-only column %s (keep_compressed = 2) is not supported: dfdb_table_decode_resident it first", what, t->cols[(size_t)e.col].name.c_str());
  return need_resident(t, e.col);
}

namespace {
// the sort's device memory: taken from the pool, back to it when the call ends (the stream drained first)
struct SortScratch {
  dfdb_ctx* ctx;
  DevBuf keys[2], rows[2], miss_rows, tile_cnt, tile_base, scan_scratch, counts, starts, hist, stage;
  explicit SortScratch(dfdb_ctx* c) : ctx(c) {}
  ~SortScratch() {
    (void)hipStreamSynchronize(ctx->stream);
    RecycleScope rs;
    for (DevBuf* b : {&keys[0], &keys[1], &rows[0], &rows[1], &miss_rows, &tile_cnt, &tile_base, &scan_scratch, &counts, &starts, &hist, &stage}) b->release();
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

void query_sort_indices(dfdb_query* q, int32_t p, int32_t flags, int64_t limit, int64_t* out, int64_t cap, int32_t memkind, int64_t* n, int64_t* info) {
  if (flags & ~DFDB_SORT_REV) fail(DFDB_ERR_ARGUMENT, "ArgumentError: sort flags %d (DFDB_SORT_REV is the only one)", flags);
  const Column& col = ordered_column(q, p, "sorting by");
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  if (t->nrows >= (int64_t)1 << 31) fail(DFDB_ERR_UNSUPPORTED, "sorting a table of 2^31 rows or more is not supported: the pairs carry rows in 32 bits");
  ensure_executed_checked(q);
  const bool rev = (flags & DFDB_SORT_REV) != 0, nullable = dt_nullable(col.dtype);
  const int dt = dt_base(col.dtype), nbits = select_key_bits(dt, false), nbytes = nbits / 8;
  const int64_t sel = query_count(q, -1);
  const int64_t total = limit < 0 ? sel : std::min(limit, sel);
  int64_t inf[4] = {sel, 0, 0, nbytes};
  if (n) *n = total;
  const int64_t m = std::min(total, std::max<int64_t>(cap, 0));
  if (m > 0 && !out) fail(DFDB_ERR_ARGUMENT, "ArgumentError: no output buffer");
  if (total == 0) { if (info) memcpy(info, inf, sizeof inf); return; }

  SortScratch S(ctx);
  const SortPlan P = plan_sort(q, col, rev, limit, sel);
  const int64_t ntiles = ceil_div(t->nrows, kTileRows);
  const uint64_t flip = rev ? (nbits == 64 ? ~0ull : (1ull << nbits) - 1ull) : 0ull;
  SortBuild B{};
  B.bitmap = q->bitmap.as<uint64_t>(); B.tile_counts = q->tile_counts.as<uint32_t>(); B.nrows = t->nrows;
  B.flip = flip; B.cut = P.cutkey ^ flip; B.keep = P.L == 0 ? SORT_KEEP_NONE : (P.cut ? SORT_KEEP_CUT : SORT_KEEP_ALL);
  int64_t npairs = sel;
  if (!nullable && !P.cut) B.live_base = q->prefix.as<uint64_t>();     // every selected row is kept: the selection's own scan places them
  else {                                                                // count the kept and the missing rows per tile, scan both
    S.tile_cnt.ensure((size_t)(ntiles + 8) * 4 * 2); S.tile_base.ensure((size_t)(ntiles + 8) * 8 * 2); S.scan_scratch.ensure(scan_counts_scratch_bytes(ntiles));
    B.live_cnt = S.tile_cnt.as<uint32_t>(); B.miss_cnt = B.live_cnt + (ntiles + 8);
    HIP_CHECK(hipMemsetAsync(S.tile_cnt.p, 0, (size_t)(ntiles + 8) * 4 * 2, s));
    { LaunchTimer lt(ctx, "sort_build"); launch_sort_build(s, col_ref(col), B, true); }
    uint64_t* lb = S.tile_base.as<uint64_t>(); uint64_t* mb = lb + (ntiles + 8);
    { LaunchTimer lt(ctx, "scan_counts");
      launch_scan_counts(s, B.live_cnt, lb, ntiles, S.scan_scratch.as<uint64_t>());
      launch_scan_counts(s, B.miss_cnt, mb, ntiles, S.scan_scratch.as<uint64_t>()); }
    HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, lb + ntiles, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar + 1, mb + ntiles, 8, hipMemcpyDeviceToHost, s));
    stream_wait(ctx);
    npairs = ctx->pinned_scalar[0];
    if (ctx->pinned_scalar[1] != P.nmiss || npairs < P.L) fail(DFDB_ERR_DEVICE, "sort: the build counted %lld kept and %lld missing rows, the plan has %lld and %lld",
                                                               (long long)npairs, (long long)ctx->pinned_scalar[1], (long long)P.L, (long long)P.nmiss);
    B.live_base = lb; B.miss_base = mb;
  }
  inf[1] = npairs;
  S.keys[0].ensure((size_t)std::max<int64_t>(npairs, 1) * 8); S.rows[0].ensure((size_t)std::max<int64_t>(npairs, 1) * 4);
  S.miss_rows.ensure((size_t)std::max<int64_t>(P.nmiss, 1) * 4);
  S.hist.ensure((size_t)(kSelectMaxRanks * 256 + 8) * 8);
  B.keys = S.keys[0].as<uint64_t>(); B.rows = S.rows[0].as<uint32_t>(); B.cap = npairs;
  B.miss_rows = S.miss_rows.as<uint32_t>(); B.miss_cap = P.nmiss;
  B.ghist = (unsigned long long*)S.hist.p;
  HIP_CHECK(hipMemsetAsync(S.hist.p, 0, (size_t)nbytes * 256 * 8, s));
  { LaunchTimer lt(ctx, "sort_build"); launch_sort_build(s, col_ref(col), B, false); }

  // a byte whose histogram has a single non-zero bin orders nothing: its pass is not run
  int cur = 0;
  if (npairs > 1) {
    std::vector<uint64_t> gh((size_t)nbytes * 256);
    HIP_CHECK(hipMemcpyAsync(gh.data(), S.hist.p, gh.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));              // (`gh` is pageable host memory)
    const int64_t nchunks = sort_chunks(npairs);
    for (int b = 0; b < nbytes; b++) {
      int used = 0;
      for (int d = 0; d < 256; d++) used += gh[(size_t)b * 256 + (size_t)d] != 0;
      if (used <= 1) continue;
      if (!S.keys[1].p) {
        S.keys[1].ensure((size_t)npairs * 8); S.rows[1].ensure((size_t)npairs * 4);
        S.counts.ensure((size_t)(256 * nchunks + 8) * 4); S.starts.ensure((size_t)(256 * nchunks + 8) * 8); S.scan_scratch.ensure(scan_counts_scratch_bytes(256 * nchunks));
      }
      { LaunchTimer lt(ctx, "sort_count"); launch_sort_count(s, S.keys[cur].as<uint64_t>(), npairs, 8 * b, S.counts.as<uint32_t>()); }
      { LaunchTimer lt(ctx, "scan_counts"); launch_scan_counts(s, S.counts.as<uint32_t>(), S.starts.as<uint64_t>(), 256 * nchunks, S.scan_scratch.as<uint64_t>()); }
      { LaunchTimer lt(ctx, "sort_scatter");
        launch_sort_scatter(s, S.keys[cur].as<uint64_t>(), S.rows[cur].as<uint32_t>(), npairs, 8 * b, S.starts.as<uint64_t>(), S.keys[cur ^ 1].as<uint64_t>(),
                            S.rows[cur ^ 1].as<uint32_t>()); }
      cur ^= 1;
      inf[2]++;
    }
  }
  inf[3] = nbytes - inf[2];

  // the first `total` of: the sorted live rows, the missing rows behind them (REV: before them) in table order; `m` of them fit the caller's buffer
  const int64_t miss_out = rev ? std::min(total, P.nmiss) : total - std::min(total, P.nlive), live_out = total - miss_out;
  int64_t* dst = out;
  if (memkind != DFDB_MEM_DEVICE && m > 0) { S.stage.ensure((size_t)m * 8); dst = S.stage.as<int64_t>(); }
  const int64_t first_n = std::min(m, rev ? miss_out : live_out), second_n = m - first_n;
  const uint32_t* live_rows = S.rows[cur].as<uint32_t>();
  { LaunchTimer lt(ctx, "sort_emit");
    launch_sort_emit(s, rev ? S.miss_rows.as<uint32_t>() : live_rows, first_n, dst, t->row_base);
    launch_sort_emit(s, rev ? live_rows : S.miss_rows.as<uint32_t>(), second_n, dst + first_n, t->row_base); }
  if (memkind != DFDB_MEM_DEVICE && m > 0) { HIP_CHECK(hipMemcpyAsync(out, dst, (size_t)m * 8, hipMemcpyDeviceToHost, s)); stream_wait(ctx); }
  if (info) memcpy(info, inf, sizeof inf);
}

void query_gather_rows(dfdb_query* q, const int64_t* rows, int64_t n, int32_t rows_memkind, dfdb_outcol* outs, int32_t ncols) {
  if (ncols != (int32_t)q->proj.size()) fail(DFDB_ERR_ARGUMENT, "ArgumentError: view has %zu columns, %d outputs given", q->proj.size(), ncols);
  if (n < 0) fail(DFDB_ERR_ARGUMENT, "ArgumentError: %lld rows", (long long)n);
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  std::vector<const Column*> cols;
  for (int32_t p = 0; p < ncols; p++) cols.push_back(&ordered_column(q, p, "gathering rows of"));
  for (int32_t p = 0; p < ncols; p++) {
    outs[p].dtype = q->proj[(size_t)p].expr->dtype; outs[p].count = n; outs[p].nbytes = 0;
    if (n > 0 && !outs[p].data) fail(DFDB_ERR_ARGUMENT, "output column %d has no data buffer", p);
  }
  if (n == 0) return;
  DevBuf rows_dev, flag;
  const int64_t* drows = rows;
  if (rows_memkind != DFDB_MEM_DEVICE) {
    rows_dev.ensure((size_t)n * 8);
    HIP_CHECK(hipMemcpyAsync(rows_dev.p, rows, (size_t)n * 8, hipMemcpyHostToDevice, s));
    drows = rows_dev.as<int64_t>();
  }
  flag.ensure(64);
  HIP_CHECK(hipMemsetAsync(flag.p, 0, 8, s));
  std::vector<DevBuf> stages((size_t)ncols * 2);
  for (int32_t p = 0; p < ncols; p++) {
    const Column& col = *cols[(size_t)p]; dfdb_outcol& o = outs[p];
    const bool dev = o.memkind == DFDB_MEM_DEVICE, want_missing = dt_nullable(col.dtype) && o.missing;
    const int w = dt_width(col.dtype);
    void* dst = o.data; uint8_t* md = want_missing ? o.missing : nullptr;
    if (!dev) {
      stages[(size_t)p * 2].ensure((size_t)n * w); dst = stages[(size_t)p * 2].p;
      HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)n * w, s));           // (a refused row writes nothing: the host copy must not carry pool bytes)
      if (want_missing) { stages[(size_t)p * 2 + 1].ensure((size_t)n); md = stages[(size_t)p * 2 + 1].as<uint8_t>(); HIP_CHECK(hipMemsetAsync(md, 0, (size_t)n, s)); }
    }
    { LaunchTimer lt(ctx, "gather_rows");
      launch_gather_rows(s, drows, n, col.data.p, w, dst, dt_nullable(col.dtype) ? col.missing.as<uint64_t>() : nullptr, md, t->row_base, t->nrows, flag.as<uint32_t>()); }
    if (!dev) {
      HIP_CHECK(hipMemcpyAsync(o.data, dst, (size_t)n * w, hipMemcpyDeviceToHost, s));
      if (want_missing) HIP_CHECK(hipMemcpyAsync(o.missing, md, (size_t)n, hipMemcpyDeviceToHost, s));
    }
  }
  HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, flag.p, 8, hipMemcpyDeviceToHost, s));
  stream_wait(ctx);                                  // (also: the staging buffers and a pageable `rows` die with this call)
  if (ctx->pinned_scalar[0] != 0) fail(DFDB_ERR_BOUNDS, "BoundsError: a row outside 1..%lld", (long long)(t->row_base + t->nrows));
}

}  // namespace dfdb
