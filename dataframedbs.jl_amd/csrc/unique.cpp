// unique.cpp — unique(col) and groupreduce on the device: the dictionary form, the dense form, the hash table and the radix-partitioned forms,
// and the groupreduce driver that chooses between them (moved out of query.cpp; the selection machinery it builds on stays there).
#include "engine.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace dfdb {

// unique(col) (column.jl:102-126 driving Base.unique; docs/src/index.md:171-182,479-486): the current selection is narrowed to
// the rows that hold the FIRST occurrence of their value in projection column p (isequal semantics), so count / materialize
// afterwards return the distinct values in order of first appearance.  A later reset / execute restores the full selection.
constexpr int64_t kGroupsInLds = 9216;      // groups a workgroup's LDS accumulators hold (k_unique.hip kGroupLdsBig): above it groupreduce goes by radix
// what unique leaves behind for groupreduce: the hash table {key, first row} (Strings: + where one holder's bytes are), or — integer keys of a small
// range — the first row per value; groupreduce turns the rows into group numbers in place
struct UniqueTables {
  DevBuf ent, aux, rep_off, rep_len, first, present;     // (aux: the control words, a UniqueAux — kernels.hpp)
  uint64_t cap = 0, salt = 0, lo = 0; uint32_t range = 0; bool is_str = false, dense = false;
  uint64_t span_lo = ~0ull, span_hi = 0;   // dense form: the first / last value index that is present (the table is laid out for the widest span it can hold)
  bool head_only = false;        // the dense form looked at the head of the column only (UniqueRequest::allow_head)
  bool optimistic = false;       // the rows behind the second insert chunk were not inserted (UniqueRequest::allow_optimistic)
  // UniqueRequest::group_probe: the number of distinct keys the first chunk's rows promise when it is more than 9216 — and then nothing else was done: the
  // selection is as it was, no table was finished
  int64_t group_estimate = 0;
  UniqueAux* ctl() const { return aux.as<UniqueAux>(); }
};
// what the caller of unique asks for (all off: a complete, verified table — or no table at all, where the radix form took the job)
struct UniqueRequest {
  // the dense form may look at the HEAD of the column only (groupreduce over integer keys, round 5: its accumulate pass meets every row anyway and reports a key
  // that has no group — one outside the span laid out, or one that first turns up behind the head —, in which case everything runs again over all rows)
  bool allow_head = false;
  bool defer_verify = false;     // the caller's own pass over the rows compares every String with its slot's representative (groupreduce's accumulate pass)
  // String keys, or defer_verify — if the second insert chunk (16 M rows) met no string the first (1 M rows) had not, the rest of the rows are NOT inserted: a
  // later pass meets every row anyway and reports a string that is not in the table (UniqueTables::optimistic comes back true; unique's own verify pass then
  // inserts every row, a caller with defer_verify asks again without this).  Ten brands over 5e8 rows: the insert pass 2.2 -> 0.1 ms.
  bool allow_optimistic = false;
  // the caller can reduce by radix (group_radix: more groups than LDS accumulators hold) and wants to know EARLY whether that is the case (UniqueTables::group_estimate)
  bool group_probe = false;
  bool allow_radix = true;       // the radix form of unique may take the job (it leaves no table to look keys up in: groupreduce_n's rank pass says no)
  int salt_skip = 0;             // salts already found colliding
};
static StrTable str_table(const UniqueTables& T) { return StrTable{T.ent.as<UniqueEntry>(), T.rep_off.as<uint64_t>(), T.rep_len.as<uint32_t>(), T.cap - 1, T.ctl(), T.salt}; }
// a control record (UniqueAux, RadixGroupAux) off the device, whole: fetch_aux enqueues the copy, read_aux also waits for it
template <typename Aux> static void fetch_aux(dfdb_ctx* ctx, const Aux* dev, Aux* host) { HIP_CHECK(hipMemcpyAsync(host, dev, sizeof(Aux), hipMemcpyDeviceToHost, ctx->stream)); }
template <typename Aux> static Aux read_aux(dfdb_ctx* ctx, const Aux* dev) { Aux h; fetch_aux(ctx, dev, &h); stream_wait(ctx); return h; }
// before a pass that may raise it
static void clear_abort(dfdb_ctx* ctx, KeyAux* head) { HIP_CHECK(hipMemsetAsync(&head->abort, 0, sizeof head->abort, ctx->stream)); }
// before a migration, which counts the claims again: the claims and the abort word, which lie side by side, in one memset
static void clear_claims_and_abort(dfdb_ctx* ctx, KeyAux* head) {
  static_assert(offsetof(KeyAux, abort) == offsetof(KeyAux, claims) + sizeof head->claims, "one memset covers both");
  HIP_CHECK(hipMemsetAsync(&head->claims, 0, sizeof head->claims + sizeof head->abort, ctx->stream));
}
// K9: unique over a String column that has a dictionary — the first selected row of every code, no hash table.  Leaves what unique_impl leaves (the
// bitmap holds exactly the first occurrences, prefix scanned); rank_of_code (optional) maps a code to its group number in order of first appearance.
static int64_t dict_unique(dfdb_query* q, const Column& col, DevBuf* rank_of_code) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const int dn = col.dict_n;
  DevBuf& first = q->du_first; first.ensure((size_t)dn * 8 + 64);      // (scratch kept on the query: every hipFree synchronises the device)
  HIP_CHECK(hipMemsetAsync(first.p, 0xFF, (size_t)dn * 8, s));
  // the first 4 M rows first: a code that has a first row there can only keep it, and a dictionary's codes have usually all turned up by then (ten brands over
  // 5e8 rows: the pass over all the codes was 0.65 ms of the groupreduce's 2.8) — only if one is still without does the rest of the column get walked
  const int64_t nt = ceil_div(t->nrows, kTileRows), head = 4096;
  std::vector<uint64_t> fr((size_t)dn);
  auto walk = [&](int64_t t0, int64_t t1) {
    { LaunchTimer lt(ctx, "unique");
      launch_dict_first_rows(s, q->bitmap.as<uint64_t>(), col.dict_codes.as<uint16_t>(), t->nrows, first.as<uint64_t>(), dn, t0, t1); }
    HIP_CHECK(hipMemcpyAsync(fr.data(), first.p, (size_t)dn * 8, hipMemcpyDeviceToHost, s));
    stream_wait(ctx);
  };
  if (nt > 4 * head) {
    walk(0, head);
    bool all = true;
    for (int k = 0; k < dn; k++) all = all && fr[(size_t)k] != ~0ull;
    if (!all) walk(head, nt);
  } else walk(0, nt);
  std::vector<std::pair<uint64_t, uint32_t>> present;
  for (int k = 0; k < dn; k++) if (fr[(size_t)k] != ~0ull) present.emplace_back(fr[(size_t)k], (uint32_t)k);
  std::sort(present.begin(), present.end());
  const int64_t ng = (int64_t)present.size();
  std::vector<uint64_t> rows((size_t)std::max<int64_t>(ng, 1));
  std::vector<uint32_t> rank((size_t)dn, 0xffffffffu);
  for (int64_t g = 0; g < ng; g++) { rows[(size_t)g] = present[(size_t)g].first; rank[present[(size_t)g].second] = (uint32_t)g; }
  DevBuf& drows = q->du_rows; drows.ensure(rows.size() * 8 + 64);
  HIP_CHECK(hipMemcpyAsync(drows.p, rows.data(), rows.size() * 8, hipMemcpyHostToDevice, s));
  if (rank_of_code) { rank_of_code->ensure(rank.size() * 4 + 64); HIP_CHECK(hipMemcpyAsync(rank_of_code->p, rank.data(), rank.size() * 4, hipMemcpyHostToDevice, s)); }
  HIP_CHECK(hipMemsetAsync(q->bitmap.p, 0, padded_words(t->nrows) * 8, s));
  HIP_CHECK(hipMemsetAsync(q->tile_counts.p, 0, (size_t)ceil_div(t->nrows, kTileRows) * 4, s));
  launch_set_rows(s, drows.as<uint64_t>(), (int)ng, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>());
  scan_prefix(q);
  selection_changed(q); q->left.cap_col = -1; q->left.cap_col2 = -1; q->left.cap_str_col = -1; q->left.agg_col = -1; q->left.const_str_col = -1;
  stream_wait(ctx);                                        // rows / rank are pageable host memory
  return ng;
}
static void unique_reset_aux(dfdb_ctx* ctx, DevBuf& buf) {
  hipStream_t s = ctx->stream;
  buf.ensure(sizeof(UniqueAux));
  UniqueAux* aux = buf.as<UniqueAux>();
  HIP_CHECK(hipMemsetAsync(aux, 0, sizeof(UniqueAux), s));
  HIP_CHECK(hipMemsetAsync(aux->head.special_row, 0xFF, sizeof aux->head.special_row, s));      // no such row yet
  HIP_CHECK(hipMemsetAsync(&aux->min_image, 0xFF, sizeof aux->min_image, s));                   // the running minimum (k_dense_minmax)
  HIP_CHECK(hipMemsetAsync(&aux->span_lo, 0xFF, sizeof aux->span_lo, s));                       // the smallest present value index (k_dense_count)
}
static uint64_t pow2_at_least(uint64_t n) { uint64_t c = 1024; while (c < n) c <<= 1; return c; }

// How many slots the table should have before the next chunk: `d` distinct keys met in the first `r` selected rows, `remaining` rows to come.
// If the rows so far were nearly all different nothing can be said (every remaining row may bring a key).  Otherwise the distinct count D of the whole
// selection is estimated as if keys were drawn uniformly — d = D (1 - exp(-r / D)), solved for D — and doubled: skewed data has more rare keys than that,
// and an estimate that turns out too small costs one more migration (or an aborted chunk), never a wrong result.
static uint64_t unique_capacity_wanted(uint64_t d, uint64_t r, uint64_t remaining, uint64_t cap, uint64_t capmax) {
  if (remaining == 0 || r == 0) return cap;
  double need;
  if ((double)d > 0.95 * (double)r) need = (double)d + (double)remaining;
  else {
    double lo = (double)(d ? d : 1), hi = 20.0 * (double)r;
    for (int it = 0; it < 64; it++) { const double D = 0.5 * (lo + hi); if (D * (1.0 - std::exp(-(double)r / D)) < (double)d) lo = D; else hi = D; }
    need = std::min((double)d + (double)remaining, 2.0 * hi + 1024.0);
  }
  const uint64_t want = pow2_at_least((uint64_t)(2.0 * need));
  return std::min(std::max(want, cap), capmax);
}

// integer keys whose selected values span less than the dense form's range (k_unique.hip, last section).  false: the span is too wide
static bool unique_dense(dfdb_query* q, const Column& col, const UniqueRequest& R, UniqueTables& T) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const int dt = dt_base(col.dtype);
  const int64_t limit = std::min<int64_t>(unique_dense_max_range(), ctx_option(ctx, "unique_dense_range", unique_dense_max_range()));
  const ColRef key = col_ref(col);
  const uint64_t flip = dt_issigned(dt) ? (1ull << 63) : 0ull;
  UniqueAux* aux = nullptr;
  uint64_t distinct = 0;
  const int64_t nt_all = ceil_div(t->nrows, kTileRows), head_tiles = std::max<int64_t>(1, ctx_option(ctx, "dense_head_tiles", 4096));
  T.head_only = R.allow_head && nt_all >= 8 * head_tiles;               // (the sample below still looks at the whole column: the span is laid around what IT saw)
  auto prows = [&]() -> int64_t { return T.head_only ? head_tiles * kTileRows : t->nrows; };      // the rows the presence pass and the first-row launches walk
  auto minmax = [&](int64_t tile_step, uint64_t* mm) {                 // order-preserving images of the smallest / largest selected key (of every tile_step-th tile)
    unique_reset_aux(ctx, T.aux);
    { LaunchTimer lt(ctx, "unique_minmax"); launch_dense_minmax(s, q->bitmap.as<uint64_t>(), key, t->nrows, tile_step, T.ctl()); }
    const UniqueAux a = read_aux(ctx, T.ctl());
    mm[0] = a.min_image; mm[1] = a.max_image;
  };
  auto presence = [&](uint64_t lo_im, uint64_t span) -> bool {         // false: a selected key lies outside [lo, lo + span]
    T.lo = lo_im ^ flip; T.range = (uint32_t)(span + 1);
    const size_t words = ((size_t)T.range + 31) / 32;
    T.first.ensure((size_t)T.range * 8 + 64); T.present.ensure(words * 4 + 64);
    HIP_CHECK(hipMemsetAsync(T.first.p, 0xFF, (size_t)T.range * 8, s));
    HIP_CHECK(hipMemsetAsync(T.present.p, 0, words * 4, s));
    unique_reset_aux(ctx, T.aux);
    aux = T.ctl();
    { LaunchTimer lt(ctx, "unique_presence");
      launch_dense_presence(s, q->bitmap.as<uint64_t>(), key, prows(), T.lo, T.range, T.present.as<uint32_t>(), aux); }
    const UniqueAux a = read_aux(ctx, aux);
    distinct = a.distinct;
    T.span_lo = a.span_lo; T.span_hi = a.span_hi;
    return a.outside == 0;
  };
  const int64_t nt = ceil_div(t->nrows, kTileRows);
  bool placed = false;
  if (dt_width(dt) <= 2) {                                             // the type's own range fits
    const int bits = dt_width(dt) * 8;
    if ((1ull << bits) > (uint64_t)limit) return false;
    placed = presence(dt_issigned(dt) ? ((uint64_t)(-(int64_t)(1ull << (bits - 1))) ^ flip) : 0ull, (1ull << bits) - 1);
  } else {
    // where the keys lie is not known.  A SAMPLE (every nt/256-th tile) says where to expect them: the whole span the form can hold is laid around the sample's
    // range and the presence pass reports any key outside it — then, and for a small table, the exact range costs a pass of its own (1.3 ms per 1e9 rows)
    uint64_t mm[2];
    const int64_t sample_opt = ctx_option(ctx, "unique_dense_sample", 1);
    const int64_t sample_step = sample_opt == 2 ? std::max<int64_t>(2, nt / 256) : nt / 256;      // (2: a sample even of a small table, every other tile — tests of what follows a sample)
    if ((sample_step >= 16 || sample_opt == 2) && sample_opt != 0) {
      minmax(sample_step, mm);
      if (mm[0] <= mm[1]) {
        if (mm[1] - mm[0] >= (uint64_t)limit) return false;
        const uint64_t slack = ((uint64_t)limit - 1 - (mm[1] - mm[0])) / 2;
        uint64_t lo_im = mm[0] > slack ? mm[0] - slack : 0ull;
        if (lo_im > ~0ull - ((uint64_t)limit - 1)) lo_im = ~0ull - ((uint64_t)limit - 1);
        placed = presence(lo_im, (uint64_t)limit - 1);
      }
    }
    if (!placed) {
      T.head_only = false;                                              // (no sample, or a key outside what it suggested: the exact range, every row)
      minmax(1, mm);
      if (mm[0] > mm[1]) mm[0] = mm[1] = flip;                         // every selected key is missing
      if (mm[1] - mm[0] >= (uint64_t)limit) return false;
      placed = presence(mm[0], mm[1] - mm[0]);
    }
  }
  if (!placed) fail(DFDB_ERR_DEVICE, "unique: a key outside the range of its column");
  T.dense = true;
  { LaunchTimer lt(ctx, "unique_first");
    // launches of 1 M, 1 M, 2 M, 4 M rows, then four times the last: every row whose value has no first row yet costs an atomic, and rows that run side by side
    // cannot see each other's — 1e6 values spread over the column are all met within 20 M rows, and met in small steps they cost 1.5 M atomics instead of 4 M
    const bool sched_default = ctx_option(ctx, "unique_chunk_tiles", 0) <= 0;
    int64_t step = sched_default ? 1024 : ctx_option(ctx, "unique_chunk_tiles", 0);
    int launches = 0;
    const int64_t nt_walk = T.head_only ? head_tiles : nt;
    int64_t t0 = 0;
    auto walk = [&](int64_t a, int64_t b) {
      launch_dense_first(s, q->bitmap.as<uint64_t>(), key, a * kTileRows, std::min(prows(), b * kTileRows), T.lo, T.range, distinct, T.first.as<uint64_t>(), aux);
    };
    // FEW values: the first 1 M rows in three steps of 16, 112 and 896 tiles — rows that run side by side all see "no first row yet" and all send their atomicMin,
    // and with seven values those are a million atomics on seven words (2.1 ms: `tools/r5_fewgroups.py`); after sixteen tiles every value has its row and the
    // launches that follow return at once
    if (sched_default && distinct <= 4096 && nt_walk >= 1024) {
      for (int64_t pre : {(int64_t)16, (int64_t)112, (int64_t)896}) { walk(t0, t0 + pre); t0 += pre; }
      launches = 1;
    }
    for (; t0 < nt_walk; t0 += step, step *= (++launches < 2 ? 1 : (launches < 4 ? 2 : 4))) walk(t0, t0 + step);
  }
  HIP_CHECK(hipMemsetAsync(q->bitmap.p, 0, padded_words(t->nrows) * 8, s));
  HIP_CHECK(hipMemsetAsync(q->tile_counts.p, 0, (size_t)ceil_div(t->nrows, kTileRows) * 4, s));
  { LaunchTimer lt(ctx, "unique_mark"); launch_dense_scatter(s, T.first.as<uint64_t>(), T.range, aux, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>()); }
  const UniqueAux a = read_aux(ctx, aux);
  if (a.outside != 0 || a.distinct != a.found) fail(DFDB_ERR_DEVICE, "unique: the dense form lost a key (outside %llu, distinct %llu, found %llu)", (unsigned long long)a.outside, (unsigned long long)a.distinct, (unsigned long long)a.found);
  return true;
}

// DevBuf::ensure for scratch the radix forms can do without: false on "no room" (the caller goes on with the older form)
static bool try_ensure(DevBuf& b, size_t bytes) {
  try { b.ensure(bytes); return true; } catch (const Error& e) { if (e.code != DFDB_ERR_NOMEM) throw; (void)hipGetLastError(); return false; }
}
// one call's scratch: back to the buffer pool when the call ends, the stream drained first (a kernel may still read it)
struct PooledScratch {
  dfdb_ctx* ctx; DevBuf buf;
  explicit PooledScratch(dfdb_ctx* c) : ctx(c) {}
  ~PooledScratch() { (void)hipStreamSynchronize(ctx->stream); RecycleScope rs; buf.release(); }
};
// The radix-partitioned form of the general unique (k_radix.hip, round 6): when the hash table would outgrow the L2s — `d0` distinct values among the first `r0`
// selected rows say how many the whole selection holds, assuming they turn up evenly: d0 = D (1 - exp(-r0 / D)) — every selected row is written once as a
// {key image, row} record into one of P partitions (by the top bits of the key's hash) and each partition is reduced through a table in LDS.  Streams instead
// of one random line per row.  false = not taken (too few or too many distinct values, no room for the 12 bytes per selected row, a partition that outgrew
// its table): the caller goes on with the hash table; the selection is as it was.
// What the two radix forms (unique, groupreduce) share on the host: the pool of pages for `nsel` records in 2^kbits partitions (k_radix.hip), its control words —
// the sample's counts [P], the streams' running positions [P x share], the pool's counter, the hot keys' count, then `extra` bytes the caller lays out (64-byte aligned) — and the hot keys'
// list.  The temporaries go back to the buffer pool (not through hipFree, which drains the device: 1.5 ms of a 16-ms call once), the stream drained first; the
// records' scratch stays with the context between calls (hipMalloc / hipFree of 12 GB cost 3-4 ms; buffers above 1 GB never enter the pool; dfdb_ctx_destroy
// releases it) unless it is more than a quarter of the device's memory.
struct RadixRun {
  dfdb_ctx* ctx; int kbits, P, C; int64_t PS; RadixPool pool{}; DevBuf ctl, pt, hot; size_t tail = 0;
  RadixRun(dfdb_ctx* c, int kb) : ctx(c), kbits(kb), P(1 << kb), C((int)round_up(4 * std::max(1, c->prop.multiProcessorCount), radix_share())), PS((int64_t)(1 << kb) * radix_share()) {}
  ~RadixRun() {
    (void)hipStreamSynchronize(ctx->stream);
    { RecycleScope rs; ctl.release(); pt.release(); hot.release(); }
    if (ctx->radix_recs.bytes > ctx->prop.totalGlobalMem / 4) ctx->radix_recs.release();
  }
  char* extra() const { return (char*)ctl.p + tail; }
  // false: no room, or more records than a 32-bit place in the pool can name
  bool prepare(int64_t nsel, bool with_values, size_t extra_bytes) {
    if (radix_pool_pages(nsel, kbits) * 8192 >= (1ll << 32)) return false;
    pool.maxv = radix_pool_maxv(nsel, kbits);
    pool.dump_page = (uint32_t)(radix_pool_pages(nsel, kbits) - 1);
    pool.hot_cap = (uint32_t)C * (uint32_t)radix_hot_slots();
    const size_t ctl_words = (size_t)P + (size_t)PS + 16;                 // the sample's counts [P], the streams' running positions [PS], the pool's counter, the hot keys' count
    tail = (ctl_words * 4 + 63) / 64 * 64;
    if (!try_ensure(ctl, tail + extra_bytes + 64) || !try_ensure(pt, (size_t)PS * pool.maxv * 4 + 512) ||      // (+ 64 entries nobody owns: the table passes read 64 at a time)
        !try_ensure(hot, (size_t)pool.hot_cap * 24 + 64) || !try_ensure(ctx->radix_recs, (size_t)radix_pool_record_bytes(nsel, kbits, with_values) + 256)) return false;
    pool.front = ctl.as<uint32_t>() + P; pool.next_page = ctl.as<uint32_t>() + P + PS; pool.hot_n = ctl.as<uint32_t>() + P + PS + 1; pool.pt = pt.as<uint32_t>(); pool.hot = hot.as<uint64_t>();
    HIP_CHECK(hipMemsetAsync(ctl.p, 0, tail + extra_bytes, ctx->stream));
    HIP_CHECK(hipMemsetAsync(pt.p, 0xFF, (size_t)PS * pool.maxv * 4, ctx->stream));
    return true;
  }
  // unique: does some partition hold a large part of all the rows (a value that a third of the column has)?  Every 16th tile is counted (all of them in a small
  // table: 0.1 ms per 1e9 rows) and the counts come back.  1 = skewed, 0 = not, -1 = the sample could not be launched
  RadixGrid grid() const { return RadixGrid{kbits, C}; }
  int skewed(const uint64_t* sel, const ColRef& key, int64_t nrows, int times) {      // times: "large" = more than this many average partitions
    const int step = radix_rows_per_chunk(nrows, C) / 8192 >= 32 ? 16 : 1;
    { LaunchTimer lt(ctx, "radix_sample");
      if (!launch_radix_sample(ctx->stream, sel, key, nrows, grid(), step, ctl.as<uint32_t>())) return -1; }
    std::vector<uint32_t> cn((size_t)P);
    HIP_CHECK(hipMemcpyAsync(cn.data(), ctl.p, (size_t)P * 4, hipMemcpyDeviceToHost, ctx->stream));
    stream_wait(ctx);
    uint64_t maxp = 0, total = 0;
    for (int p = 0; p < P; p++) { maxp = std::max<uint64_t>(maxp, cn[(size_t)p]); total += cn[(size_t)p]; }
    return maxp * (uint64_t)step > 65536 && maxp * (uint64_t)P > (uint64_t)times * total ? 1 : 0;
  }
};
// how many distinct values `cnt` selected rows hold when the first r0 of them held d0, assuming they turn up evenly: d0 = D (1 - exp(-r0 / D)), by bisection
static double estimate_distinct(uint64_t d0, uint64_t r0, int64_t cnt) {
  double D = (double)cnt;
  if (d0 < r0) {
    double lo = (double)d0, hi = (double)cnt;
    for (int it = 0; it < 60 && hi - lo > 1.0; it++) { const double mid = 0.5 * (lo + hi); if (mid * (1.0 - std::exp(-(double)r0 / mid)) < (double)d0) lo = mid; else hi = mid; }
    D = std::min((double)cnt, hi);
  }
  return D;
}
static bool unique_radix(dfdb_query* q, const Column& col, int64_t cnt, UniqueTables& T, uint64_t d0, uint64_t r0) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  // MEASURED, 1e9 Int64 / Float64 rows of 1e6 distinct values (profiles/r6_unique_radix.txt): sample 0.1 + partition 4.5 + LDS tables 3.2 ms = 8.8-9.3 ms end to end against the
  // hash table's 19.8 (the first build, with splitmix64, a counting pass and the partition re-hashed on the way out, was 18.4).  The partition pass waits for its STORES
  // (2.8 ms without them): 192-byte runs behind running positions that one XCD's workgroups share, so that whole lines leave that XCD's L2.  On by default; option = 0: the hash table.
  const int64_t mode = ctx_option(ctx, "unique_radix", 1);
  if (mode == 0 || t->nrows >= (1ll << 32) - 8192 || r0 == 0 || d0 == 0) return false;      // (rows and pool positions are 32-bit; all ones is "no row")
  if (mode < 2 && cnt < (4ll << 20)) return false;                       // (2: a test knob — any size; measured against the hash table down to 3 M selected rows of 1e9: tools/r6_radix_selective.py)
  const double D = estimate_distinct(d0, r0, cnt);
  if (mode < 2 && D < 131072.0) return false;                            // the hash table stays in the L2s: nothing to gain
  int kbits = 8;
  while (kbits < 10 && D / (double)(1 << kbits) > 2500.0) kbits++;       // (fewer partitions = longer runs per tile of the partition pass; more = emptier tables in the unique pass: 1e6 values -> 512)
  if (mode < 2 && D / (double)(1 << kbits) > 5500.0) return false;       // the partitions' tables (8192 slots) would overflow
  const ColRef key = col_ref(col);
  const int64_t nt = ceil_div(t->nrows, kTileRows);
  const size_t nw = padded_words(t->nrows);
  PooledScratch keep_sel(ctx), keep_tc(ctx);                             // the selection, set aside
  DevBuf &sel_keep = keep_sel.buf, &tc_keep = keep_tc.buf;
  RadixRun run(ctx, kbits);
  if (!run.prepare(cnt, false, 0) || !try_ensure(sel_keep, nw * 8) || !try_ensure(tc_keep, (size_t)nt * 4 + 64)) return false;
  const RadixPool& pool = run.pool;
  DevBuf& recs = ctx->radix_recs;
  // SKEW: one workgroup reduces one partition, so a value that a large part of the rows hold would be one CU's work while 255 wait.  The sample says whether some
  // partition holds more than eight average ones; then the partition kernels that keep hot keys out of the records run (k_radix.hip, hot keys: 1.1 ms slower where
  // nothing is hot, which is why they are not the only ones)
  const int sk = run.skewed(q->bitmap.as<uint64_t>(), key, t->nrows, 8);
  if (sk < 0) return false;
  if (sk) prof_note(ctx, "unique_radix.skewed");
  { LaunchTimer lt(ctx, "radix_partition");
    if (!launch_radix_partition(s, q->bitmap.as<uint64_t>(), key, t->nrows, run.grid(), pool, recs.as<uint32_t>(), &T.ctl()->head, nullptr, sk != 0)) return false; }
  // the selection is set aside (a partition that outgrows its table means: back to the hash table, over the same selection)
  HIP_CHECK(hipMemcpyAsync(sel_keep.p, q->bitmap.p, nw * 8, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(tc_keep.p, q->tile_counts.p, (size_t)nt * 4, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemsetAsync(q->bitmap.p, 0, nw * 8, s));
  HIP_CHECK(hipMemsetAsync(q->tile_counts.p, 0, (size_t)nt * 4, s));
  bool ok;
  { LaunchTimer lt(ctx, "radix_unique");
    ok = launch_radix_unique(s, recs.as<uint32_t>(), pool, kbits, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), &T.ctl()->head, ctx->prop.multiProcessorCount); }
  const uint64_t aborted = ok ? read_aux(ctx, T.ctl()).head.abort : 0;
  if (!ok || aborted || ctx_option(ctx, "unique_radix", 1) == 3) {        // (3: a test knob — behave as if a partition had overflowed)
    HIP_CHECK(hipMemcpyAsync(q->bitmap.p, sel_keep.p, nw * 8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(q->tile_counts.p, tc_keep.p, (size_t)nt * 4, hipMemcpyDeviceToDevice, s));
    clear_abort(ctx, &T.ctl()->head);
    stream_wait(ctx);
    prof_note(ctx, "unique_radix.fell_back");
    return false;
  }
  prof_note(ctx, "unique_radix.taken");
  stream_wait(ctx);                                                      // (the temporaries die with this frame)
  return true;
}

// the general form: an open-addressing table of {key, first row} sized by the distinct values as they turn up (k_unique.hip)
static void unique_hashed(dfdb_query* q, const Column& col, int64_t cnt, const UniqueRequest& R, UniqueTables& T) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const bool is_str = T.is_str;
  const ColRef key = is_str ? ColRef{} : col_ref(col);                 // (a flat String key travels as str_side(col) + str_table(T))
  const int64_t nt = ceil_div(t->nrows, kTileRows);
  const uint64_t capmax = pow2_at_least((uint64_t)cnt * 2);
  const uint64_t cap0 = std::min(capmax, pow2_at_least(1ull << std::min<int64_t>(40, std::max<int64_t>(10, ctx_option(ctx, "unique_cap0_log2", 21)))));
  const int64_t c0 = ctx_option(ctx, "unique_chunk_tiles", 0) > 0 ? ctx_option(ctx, "unique_chunk_tiles", 0) : 1024;
  const int64_t bounds[3] = {std::min(nt, c0), std::min(nt, c0 * 17), nt};
  auto alloc = [&](UniqueTables& U, uint64_t cap) {
    U.cap = cap;
    U.ent.ensure(cap * sizeof(UniqueEntry));
    HIP_CHECK(hipMemsetAsync(U.ent.p, 0xFF, cap * sizeof(UniqueEntry), s));
    if (is_str) { U.rep_off.ensure(cap * 8); U.rep_len.ensure(cap * 4); }
  };
  auto insert = [&](int64_t t0, int64_t t1) {
    LaunchTimer lt(ctx, "unique_insert");
    if (is_str) launch_unique_str(s, 0, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), str_side(col), t->nrows, t0, t1, str_table(T));
    else launch_unique_insert(s, q->bitmap.as<uint64_t>(), key, t0 * kTileRows, std::min(t->nrows, t1 * kTileRows), T.ent.as<UniqueEntry>(), T.cap - 1, T.ctl());
  };
  UniqueAux st{};                                                      // the control words as last read: claimed slots, abort flag
  auto read_state = [&](uint64_t* selected_before, int64_t tile) {
    fetch_aux(ctx, T.ctl(), &st);
    if (selected_before) HIP_CHECK(hipMemcpyAsync(selected_before, q->prefix.as<uint64_t>() + tile, 8, hipMemcpyDeviceToHost, s));
    stream_wait(ctx);
  };
  auto grow = [&](uint64_t cap) {                                      // the entries move to a table of `cap` slots
    LaunchTimer lt(ctx, "unique_migrate");
    UniqueTables N; N.is_str = is_str;
    alloc(N, cap);
    clear_claims_and_abort(ctx, &T.ctl()->head);
    launch_unique_migrate(s, T.ent.as<UniqueEntry>(), is_str ? T.rep_off.as<uint64_t>() : nullptr, is_str ? T.rep_len.as<uint32_t>() : nullptr, T.cap, N.ent.as<UniqueEntry>(),
                          N.rep_off.as<uint64_t>(), N.rep_len.as<uint32_t>(), cap - 1, T.ctl());
    read_state(nullptr, 0);
    if (st.head.abort) fail(DFDB_ERR_DEVICE, "unique: %llu entries do not fit a table of %llu slots", (unsigned long long)st.head.claims, (unsigned long long)cap);
    T.ent = std::move(N.ent); T.rep_off = std::move(N.rep_off); T.rep_len = std::move(N.rep_len); T.cap = cap;
  };
  T.salt = 0x51ED270B27B4F3CFull;
  for (int k = 0; k < R.salt_skip; k++) T.salt = splitmix64_host(T.salt);
  bool allow_optimistic = R.allow_optimistic;                          // (until an optimistic table turns out incomplete)
  for (int tries = R.salt_skip;; tries++, T.salt = splitmix64_host(T.salt)) {
    if (!T.ent.p || T.cap != cap0) { T.ent.release(); alloc(T, cap0); } else HIP_CHECK(hipMemsetAsync(T.ent.p, 0xFF, T.cap * sizeof(UniqueEntry), s));
    unique_reset_aux(ctx, T.aux);
    int64_t t0 = 0;
    uint64_t claims_c0 = 0, rows_c0 = 0;
    T.optimistic = false;
    // (a column of FEW keys: the rows of a chunk run side by side, all see an empty slot or a larger first row, and all send their atomic — 1 M rows on seven
    // slots took 1.1 ms.  Sixteen tiles first: after them the chunk's rows find their key with a smaller row and send nothing.  Inserts are idempotent.)
    if (bounds[0] > 64) insert(0, 16);
    for (int c = 0; c < 3; c++) {
      const int64_t t1 = bounds[c];
      if (t1 <= t0) continue;
      uint64_t r = 0;
      // (numeric keys: only for a caller whose own pass over the rows can report a key without a slot — groupreduce's accumulate pass, defer_verify —, and only when
      // the distinct keys are few beside the rows, so that the first rows come straight out of the table below)
      // (String keys too.  After an optimistic break the mark step below must take the first rows straight out of the table — launch_unique_scatter,
      // `claims * 8 <= cnt` — because the per-row mark pass looks every selected row up with an unbounded probe, and a row of the un-inserted tail whose
      // string the table does not hold would never leave that loop: a GPU hang, which no host-side guard can catch.)
      if (c == 2 && (is_str || R.defer_verify) && allow_optimistic && claims_c0 != ~0ull && st.head.claims * 8 <= (uint64_t)cnt) { T.optimistic = true; break; }
      for (;;) {
        insert(t0, t1);
        read_state(&r, t1);
        if (!st.head.abort) break;
        if (T.cap >= capmax) fail(DFDB_ERR_DEVICE, "unique: probe sequences of a half-empty table got too long (%llu slots, %llu keys)", (unsigned long long)T.cap, (unsigned long long)st.head.claims);
        grow(std::min(capmax, T.cap * 4));                             // (that clears the flag) and the chunk again: inserts are idempotent
      }
      // (optimistic: chunk 1 must have fed at least 64 K selected rows and claimed nothing that chunk 0 had not)
      if (c == 0) { claims_c0 = st.head.claims; rows_c0 = r; }
      else if (c == 1 && !(st.head.claims == claims_c0 && r >= rows_c0 + 65536)) claims_c0 = ~0ull;
      if (c == 0 && !is_str) {
        if (R.group_probe && r > 0) {                                  // groupreduce asks: more groups than LDS accumulators hold?  Then it reduces by radix, first rows included
          const double D = estimate_distinct(st.head.claims, r, cnt);
          if (D > (double)kGroupsInLds) { T.group_estimate = (int64_t)D; return; }
        }
        if (!R.defer_verify && R.allow_radix && unique_radix(q, col, cnt, T, st.head.claims, r)) return;      // the radix-partitioned form took it: q's bitmap holds the first occurrences
      }
      if (c == 0 && bounds[1] <= bounds[0]) claims_c0 = ~0ull;
      const uint64_t want = unique_capacity_wanted(st.head.claims, r, (uint64_t)cnt - std::min<uint64_t>(r, (uint64_t)cnt), T.cap, capmax);
      if (want > T.cap) grow(want);
      t0 = t1;
    }
    if (!is_str || R.defer_verify) break;
    // the pass that compares every selected row with its slot's representative.  After an optimistic insert it also meets the rows that were never inserted: a string
    // the table does not hold raises the abort word and everything runs again with every row inserted (as groupreduce's accumulate pass does it)
    if (T.optimistic) clear_abort(ctx, &T.ctl()->head);
    launch_unique_str(s, T.optimistic ? 3 : 1, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), str_side(col), t->nrows, 0, nt, str_table(T));
    const UniqueAux v = read_aux(ctx, T.ctl());
    if (T.optimistic && (v.head.abort != 0 || ctx_option(ctx, "groupreduce_optimistic", 1) == 2)) { allow_optimistic = false; continue; }   // (2: the test knob, as in groupreduce)
    if (!(uint32_t)v.collision) break;                                 // no two different strings shared a key: the table is exact
    if (tries >= 8) fail(DFDB_ERR_DEVICE, "unique: hash collisions under 8 different salts");
  }
  LaunchTimer lt(ctx, "unique_mark");
  if (st.head.claims * 8 <= (uint64_t)cnt) {                           // few distinct values beside the rows: the first rows straight out of the table
    HIP_CHECK(hipMemsetAsync(q->bitmap.p, 0, padded_words(t->nrows) * 8, s));
    HIP_CHECK(hipMemsetAsync(q->tile_counts.p, 0, (size_t)nt * 4, s));
    launch_unique_scatter(s, T.ent.as<UniqueEntry>(), T.cap, T.ctl(), q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>());
  } else if (is_str) {
    launch_unique_str(s, 2, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), str_side(col), t->nrows, 0, nt, str_table(T));
  } else {
    launch_unique_mark(s, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), key, t->nrows, T.ent.as<UniqueEntry>(), T.cap - 1, T.ctl());
  }
}

// (col: a column of the table, or a transient one that belongs to no table's column list — groupreduce_n's images)
static void unique_impl_col(dfdb_query* q, const Column& col, const UniqueRequest& R, UniqueTables* keep) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx;
  const int64_t cnt = query_count(q, -1);
  if (cnt == 0 || t->nrows == 0) return;
  if (!keep && col.dict_n > 0) { dict_unique(q, col, nullptr); return; }
  UniqueTables local;
  UniqueTables& T = keep ? *keep : local;
  T.is_str = dt_base(col.dtype) == DFDB_STRING; T.dense = false; T.group_estimate = 0;
  {
    LaunchTimer lt(ctx, "unique");
    const bool dense = !T.is_str && unique_dense_dtype(dt_base(col.dtype)) && ctx_option(ctx, "unique_dense", 1) != 0 && unique_dense(q, col, R, T);
    if (!dense) unique_hashed(q, col, cnt, R, T);
  }
  scan_prefix(q);
  selection_changed(q); q->left.cap_col = -1; q->left.cap_col2 = -1; q->left.cap_str_col = -1; q->left.agg_col = -1;
  stream_wait(ctx);                                        // the tables die here (or stay with the caller: groupreduce looks rows up in them)
  if (!keep) { RecycleScope rs; local = UniqueTables(); }
}
static void unique_impl(dfdb_query* q, int32_t p, const UniqueRequest& R, UniqueTables* keep) {
  ensure_executed_checked(q);
  if (p < 0 || (size_t)p >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", p);
  const Node& e = *q->proj[(size_t)p].expr;
  if (e.op != DFIR_COL) fail(DFDB_ERR_UNSUPPORTED, "unique of a computed column: materialise it as a column first (dfdb_table_add_from_query)");
  unique_impl_col(q, need_resident(q->t, e.col), R, keep);
}
void query_unique(dfdb_query* q, int32_t p) {
  UniqueRequest R;
  R.allow_optimistic = ctx_option(q->t->ctx, "groupreduce_optimistic", 1) != 0;      // (unique's own compare pass meets every row: the same bargain as groupreduce's)
  unique_impl(q, p, R, nullptr);
}

// the groups' counts (zero) and values (the identity of `op`) for `ng` groups
static void reset_group_outputs(dfdb_query* q, int64_t ng, int op) {
  hipStream_t s = q->t->ctx->stream;
  q->gr_cnt.ensure((size_t)ng * 8 + 64); q->gr_val.ensure((size_t)ng * 8 + 64);
  HIP_CHECK(hipMemsetAsync(q->gr_cnt.p, 0, (size_t)ng * 8 + 64, s));
  HIP_CHECK(hipMemsetAsync(q->gr_val.p, op == DFDB_AGG_MIN ? 0xFF : 0, (size_t)ng * 8 + 64, s));
}
// groupreduce narrowed q's bitmap to the groups' first rows: the full selection it kept aside (gr_sel) back — bitmap, tile counts, prefix
static void restore_group_selection(dfdb_query* q) {
  launch_missing_mask(q->t->ctx->stream, q->gr_sel.as<uint64_t>(), false, false, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), q->t->nrows);
  scan_prefix(q);
  selection_changed(q);
}

// groupreduce over MORE groups than a workgroup's LDS accumulators hold, by radix (k_radix.hip, round 6): with the first occurrences already in q's bitmap (unique
// made them: `ng` groups, q->prefix scanned) every selected row of `sel` is written as a {key, row, value} record into one of P partitions, each partition is reduced
// through a table in LDS, and a key's result goes to the place its first row's rank names.  false = not taken (nothing was written to the outputs): too many groups
// for the tables, a skewed column, no room — the caller's accumulate pass (global atomics) runs.  85-135 ms -> see profiles/r6_groupreduce_radix.txt.
// mark: q's bitmap does NOT hold every group's first row yet (unique looked at the head of the column only): the table pass marks them itself — the bitmap is
// cleared first, scanned afterwards, and *ng_io becomes the number of groups; on false the bitmap is whatever the pass left (the caller restores the selection).
// (key: the key column — or a dictionary's 16-bit codes as a UInt16 column)
static bool group_radix(dfdb_query* q, const ColRef& key, const Column* vc, int op, int64_t nsel, int64_t* ng_io, const uint64_t* sel, bool mark) {
  int64_t ng = mark ? *ng_io + *ng_io / 4 + 1024 : *ng_io;                // (marking: an estimate from the head — the tables are sized with room to spare)
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const int64_t mode = ctx_option(ctx, "unique_radix", 1);
  if (mode == 0 || t->nrows >= (1ll << 32) - 8192 || key.dtype == DFDB_STRING) return false;
  int kbits = 9;                                                         // (512 partitions at least: one workgroup reduces one partition, and there are 256 CUs)
  while (kbits < 10 && ng / (1ll << kbits) > 1200) kbits++;              // (a 4096-slot table at 30 % load)
  if ((mark ? *ng_io : ng) / (1ll << kbits) > 2400) return false;        // (59 % load: the claims stop a table at 7/8, and that raises the abort word)
  const int P = 1 << kbits;
  PooledScratch res(ctx);
  RadixRun run(ctx, kbits);
  if (!run.prepare(nsel, true, sizeof(RadixGroupAux)) || !try_ensure(res.buf, (size_t)(mark ? (int64_t)P * radix_group_slots() : ng) * 16 + 256)) return false;
  const RadixPool& pool = run.pool;
  DevBuf& recs = ctx->radix_recs;
  RadixGroupAux* aux = (RadixGroupAux*)run.extra();                      // (zero: prepare cleared it)
  RadixGroup g{};
  g.val = col_ref(vc);
  const int kind = q->gr_kinds_n[0];
  g.gop = op == DFDB_AGG_SUM ? (kind == 2 ? 2 : 1) : (op == DFDB_AGG_MIN ? 3 : (op == DFDB_AGG_MAX ? 4 : 0));
  if (!vc) g.gop = 0;
  g.vkind = kind; g.results = res.buf.p; g.aux = aux;
  HIP_CHECK(hipMemsetAsync(aux->head.special_row, 0xFF, sizeof aux->head.special_row, s));      // no such row yet
  if (g.gop == 3) for (int k = 0; k < 2; k++) HIP_CHECK(hipMemsetAsync(&aux->gspec[2 * k + 1], 0xFF, sizeof aux->gspec[0], s));      // the two groups' values: a minimum starts at all ones
  // a key that a large part of the rows hold is reduced by the partition pass itself (k_radix.hip, hot keys: the form this replaces sent every one of its rows
  // through a global atomic on ONE address — 3.6 s per 1e9 rows with a key that 30 % of them hold); the kernels that do so are 0.8-1.1 ms slower where nothing is
  // hot, so the sample picks: some partition above THREE average ones, and they run
  const int sk = run.skewed(sel, key, t->nrows, 3);
  if (sk < 0) return false;
  if (sk) prof_note(ctx, "group_radix.skewed");
  { LaunchTimer lt(ctx, "radix_partition");
    if (!launch_radix_partition(s, sel, key, t->nrows, run.grid(), pool, recs.as<uint32_t>(), &aux->head, &g, sk != 0)) return false; }
  if (mark) {
    HIP_CHECK(hipMemsetAsync(q->bitmap.p, 0, padded_words(t->nrows) * 8, s));
    HIP_CHECK(hipMemsetAsync(q->tile_counts.p, 0, (size_t)ceil_div(t->nrows, kTileRows) * 4, s));
  }
  { LaunchTimer lt(ctx, "radix_group");
    if (!launch_radix_group(s, recs.as<uint32_t>(), pool, kbits, mark, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), g, ctx->prop.multiProcessorCount)) return false; }
  const RadixGroupAux a = read_aux(ctx, aux);
  const uint32_t nres = (uint32_t)a.nres;
  if (a.head.abort != 0) { prof_note(ctx, "group_radix.fell_back"); return false; }
  if (mark) {
    scan_prefix(q);
    selection_changed(q);
    ng = query_count(q, -1);
    *ng_io = ng;
  }
  if ((int64_t)nres + (a.head.special_row[SPECIAL_UNSTORABLE] != ~0ull ? 1 : 0) + (a.head.special_row[SPECIAL_MISSING] != ~0ull ? 1 : 0) != ng) { prof_note(ctx, "group_radix.mismatch"); return false; }     // (cannot happen: the table pass saw every key unique saw)
  reset_group_outputs(q, ng, op);
  launch_radix_group_finish(s, g, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), q->gr_cnt.as<uint64_t>(), q->gr_val.as<uint64_t>());
  prof_note(ctx, "group_radix.taken");
  return true;                                                           // (the temporaries' destructor drains the stream)
}

// what every form of the single-reducer accumulate pass reads: the full selection (gr_sel), the value column (null: count only) and the outputs
static AccArgs group_acc_args(dfdb_query* q, const Column* vc, int op, int64_t ng, uint64_t init) {
  AccArgs A{};
  A.sel = q->gr_sel.as<uint64_t>(); A.nrows = q->t->nrows; A.value(col_ref(vc)); A.op = op;
  A.cnt = q->gr_cnt.as<uint64_t>(); A.val = q->gr_val.as<uint64_t>(); A.ngroups = (int)ng; A.val_init = init;
  return A;
}

// groupreduce by the key column's values: unique's table (hash or dense; `T` holds it when this returns) + group numbers + an accumulate pass, or the radix
// form — and all of it again over the full selection whenever a pass finds the table it was given incomplete.  Returns the number of groups, q->gr_cnt /
// gr_val filled (before launch_group_finish).
static int64_t groupreduce_hashed(dfdb_query* q, int32_t key_p, const Column& kc, const Column* vc, int op, int64_t nsel, uint64_t init, UniqueTables& T) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  int64_t ng = 0;
  bool pessimistic = false, whole_dense = false, radix_failed = false;
  int collisions = 0;                                            // salts found colliding so far
  // integer keys, dense form: the table of first rows / group numbers is made from the HEAD of the column (4 M rows) when the accumulate pass can be the one with
  // the table in LDS — that pass meets every row anyway and raises a flag for a key that has no group, after which everything runs again over every row
  // (the presence pass over the whole key column was 1.3 of the 5.0 ms of 1e9 rows by 5000 keys)
  const bool head_ok = ctx_option(ctx, "groupreduce_optimistic", 1) != 0 && (dt_base(kc.dtype) == DFDB_I64 || dt_base(kc.dtype) == DFDB_U64) &&
                       (!vc || dt_width(vc->dtype) == 8);
  for (;;) {
    // String keys: the pass that compares every row with its slot's representative (unique's verify pass) is folded into the accumulate pass below, which
    // hashes every row and finds its slot anyway; should two different strings share a key the selection is put back and everything runs again under the next salt
    UniqueRequest R;
    R.defer_verify = true;
    R.allow_optimistic = !pessimistic && ctx_option(ctx, "groupreduce_optimistic", 1) != 0;
    R.allow_head = head_ok && !whole_dense;
    R.group_probe = !radix_failed && ctx_option(ctx, "unique_radix", 1) != 0 && dt_base(kc.dtype) != DFDB_STRING;
    R.salt_skip = collisions;
    unique_impl(q, key_p, R, &T);
    if (T.group_estimate > 0) {                                  // the first chunk of rows promises more groups than any accumulate pass's LDS holds: by radix, first rows and all
      ng = T.group_estimate;
      if (group_radix(q, col_ref(kc), vc, op, nsel, &ng, q->gr_sel.as<uint64_t>(), true)) break;
      radix_failed = true;                                       // (skewed, too many groups, no room: the bitmap may have been cleared — everything again, the old way)
      restore_group_selection(q);
      continue;
    }
    const bool head_table = T.dense && T.head_only;
    UniqueAux* aux = T.ctl();
    if (head_table) clear_abort(ctx, &aux->head);        // (the word the accumulate pass raises)
    if (T.optimistic) clear_abort(ctx, &aux->head);      // the accumulate pass raises this word when it meets a string the table does not hold
    ng = query_count(q, -1);
    uint64_t* special = aux->head.special_row;
    if (T.dense) launch_dense_group_ids(s, T.first.as<uint64_t>(), T.range, aux, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>());
    else launch_group_ids(s, T.ent.as<UniqueEntry>(), T.cap, special, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>());
    reset_group_outputs(q, ng, op);
    // more groups than the LDS accumulators of any accumulate pass hold: by radix (group_radix) — which needs EVERY group's first row in the bitmap: a table made
    // from the head of the column / a prefix of the rows is made again from all of them first
    if (!radix_failed && !T.is_str && ng > kGroupsInLds && ctx_option(ctx, "unique_radix", 1) != 0 && ng <= 2400 * 1024) {
      const bool partial = head_table || T.optimistic;          // unique looked at the head of the column / a prefix of the rows: not every group's first row is marked
      if (group_radix(q, col_ref(kc), vc, op, nsel, &ng, q->gr_sel.as<uint64_t>(), partial)) break;
      radix_failed = true;
      if (partial) {                                             // not taken, and the bitmap may have been cleared: everything again, every row looked at
        whole_dense = true; pessimistic = true;
        restore_group_selection(q);     // the full selection again
        continue;
      }
    }
    int dense_lds = 0;
    { LaunchTimer lt(ctx, "group_accumulate");
      AccArgs A = group_acc_args(q, vc, op, ng, init);
      A.special = special;
      if (T.dense) {
        A.key(col_ref(kc)); A.lo = T.lo; A.gids = T.first.as<uint64_t>();
        A.unknown_flag = head_table ? &aux->head.abort : nullptr;
        dense_lds = launch_group_accumulate(s, GROUP_SRC_DENSE, A, GroupAccExtra{nullptr, T.range, T.span_lo, T.span_hi});
      } else if (T.is_str)
        launch_group_accumulate_str(s, A, str_side(kc), str_table(T));
      else {
        // few groups of an 8-byte key: their keys (the key column at the first rows q's bitmap now holds, i.e. in group order) for the accumulate pass's LDS table
        const void* gkeys = nullptr;
        if (ng <= kGroupsInLds && dt_width(kc.dtype) == 8) {
          q->gr_keys.ensure((size_t)ng * 8 + 64);
          launch_gather(s, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), kc.data.p, q->gr_keys.p, 8, t->nrows, ng);
          gkeys = q->gr_keys.p;
        }
        A.key(col_ref(kc)); A.ent = T.ent.as<UniqueEntry>(); A.mask = T.cap - 1;
        A.unknown_flag = T.optimistic ? &aux->head.abort : nullptr;      // the table was filled from a prefix of the rows: a key without a slot raises this word
        if (launch_group_accumulate(s, GROUP_SRC_HASH, A, GroupAccExtra{gkeys, 0, 0, 0}) > 0) prof_note(ctx, "group_accumulate.hash_lds");
      } }
    if (dense_lds > 0) prof_note(ctx, "group_accumulate.dense_lds");
    if (head_table) {
      uint64_t unknown = dense_lds < 0 ? 1ull : 0ull;                  // (-1: the LDS form could not take the job and nothing ran)
      if (!unknown) unknown = read_aux(ctx, aux).head.abort;
      if (unknown || ctx_option(ctx, "groupreduce_optimistic", 1) == 2) {          // (2: the test knob — as if a key had been missing)
        whole_dense = true;
        prof_note(ctx, "group_accumulate.head_redo");
        restore_group_selection(q);     // the full selection again
        continue;
      }
      prof_note(ctx, "group_accumulate.head_table");
    }
    if (!T.is_str && !T.optimistic) break;
    const UniqueAux a = read_aux(ctx, aux);
    const bool hit = (uint32_t)a.collision != 0;
    const bool redo_all = T.optimistic && (a.head.abort != 0 || ctx_option(ctx, "groupreduce_optimistic", 1) == 2);      // (2: a test knob — behave as if a string had been missing)
    if (!T.is_str && !redo_all) break;                       // (numeric keys: nothing to collide)
    if (!hit && !redo_all && ctx_option(ctx, "unique_test_collide", 0) <= collisions) break;
    if (redo_all) pessimistic = true;                         // a string first met after the inserted prefix: everything again, every row inserted
    else if (++collisions > 8) fail(DFDB_ERR_DEVICE, "unique: hash collisions under 8 different salts");
    restore_group_selection(q);     // the full selection again
  }
  return ng;
}

std::vector<int> groupreduce_check(const dfdb_query* q, const int32_t* key_cols, int32_t nkeys, const int32_t* val_cols, const int32_t* stats, int32_t nvals,
                                   const char* by_prefix) {
  if (nkeys < 1 || nkeys > 8 || !key_cols) fail(DFDB_ERR_ARGUMENT, "ArgumentError: groupreduce takes 1 to 8 key columns, not %d", nkeys);
  if (nvals < 0 || nvals > kMaxReducers || (nvals > 0 && (!val_cols || !stats))) fail(DFDB_ERR_ARGUMENT, "ArgumentError: groupreduce takes 0 to %d reducers, not %d", kMaxReducers, nvals);
  for (int k = 0; k < nkeys; k++) {
    const int32_t p = key_cols[k];
    if (p < 0 || (size_t)p >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", p);
    if (q->proj[(size_t)p].expr->op != DFIR_COL) fail(DFDB_ERR_UNSUPPORTED, "%sgroupreduce by a computed column: materialise it as a column first (dfdb_table_add_from_query)", by_prefix);
  }
  std::vector<int> kinds((size_t)nvals, 0);
  for (int m = 0; m < nvals; m++) {
    const int32_t op = stats[m];
    if (op != DFDB_AGG_COUNT && op != DFDB_AGG_SUM && op != DFDB_AGG_MIN && op != DFDB_AGG_MAX) fail(DFDB_ERR_ARGUMENT, "unknown statistic %d", op);
    if (op == DFDB_AGG_COUNT) continue;                      // (a count reads no column)
    const int32_t p = val_cols[m];
    if (p < 0 || (size_t)p >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", p);
    const Node& ve = *q->proj[(size_t)p].expr;
    if (ve.op != DFIR_COL || !dt_isnum(ve.dtype) || dt_nullable(ve.dtype)) fail(DFDB_ERR_UNSUPPORTED, "groupreduce over %s: a plain numeric column is needed", dt_name(ve.dtype).c_str());
    kinds[(size_t)m] = value_kind(dt_base(ve.dtype));
  }
  return kinds;
}
void group_values_out(const uint64_t* bits, int64_t n, int kind, int64_t* vals_i, double* vals_f) {
  for (int64_t j = 0; j < n; j++) {
    const uint64_t b = bits[j];
    double d; memcpy(&d, &b, 8);
    if (kind == 2) { if (vals_f) vals_f[j] = d; if (vals_i) vals_i[j] = (int64_t)d; }
    else { if (vals_i) vals_i[j] = (int64_t)b; if (vals_f) vals_f[j] = kind == 1 ? (double)b : (double)(int64_t)b; }
  }
}

// groupreduce(view, (:key,); out = :val => Stat()) (src/tables/aggregate.jl:1-36; unfinished in the reference: it numbers the groups in order of
// first appearance of the key and prints the map).  Completed to that intent: one group per distinct key (isequal), groups in order of first
// appearance, count and one reduced value per group.  Device side: unique's table + k_group_ids + k_group_accumulate (k_unique.hip).
void query_groupreduce(dfdb_query* q, int32_t key_p, int32_t val_p, int32_t op, int64_t* ngroups, int64_t* key_bytes) {
  ensure_executed_checked(q);
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const std::vector<int> kinds = groupreduce_check(q, &key_p, 1, &val_p, &op, 1);
  const Column* vc = op != DFDB_AGG_COUNT ? &need_resident(t, q->proj[(size_t)val_p].expr->col) : nullptr;
  const Column& kc = need_resident(t, q->proj[(size_t)key_p].expr->col);
  q->gr_n = 0; q->gr_multi = 0; q->gr_keys_n.assign(1, key_p); q->gr_ops_n.assign(1, op); q->gr_kinds_n = kinds;
  if (ngroups) *ngroups = 0;
  if (key_bytes) *key_bytes = 0;
  const int64_t nsel = query_count(q, -1);
  if (nsel == 0 || t->nrows == 0) { q->gr_state = 1; return; }
  // the full selection is kept aside: unique narrows q's bitmap to the first occurrences (= the groups, in order)
  const size_t nw = padded_words(t->nrows);
  q->gr_sel.ensure(nw * 8);
  HIP_CHECK(hipMemcpyAsync(q->gr_sel.p, q->bitmap.p, nw * 8, hipMemcpyDeviceToDevice, s));
  const uint64_t init = op == DFDB_AGG_MIN ? ~0ull : 0ull;
  UniqueTables T;
  int64_t ng;
  if (kc.dict_n > 0) {                                       // K9: group by the dictionary codes
    DevBuf& rank = q->du_rank;
    ng = dict_unique(q, kc, &rank);
    // more codes in use than LDS accumulators hold: the codes are the keys of the radix form (the first occurrences are in the bitmap already)
    if (!(ng > kGroupsInLds && group_radix(q, ColRef{kc.dict_codes.p, DFDB_U16, nullptr}, vc, op, nsel, &ng, q->gr_sel.as<uint64_t>(), false))) {
      reset_group_outputs(q, ng, op);
      LaunchTimer lt(ctx, "group_accumulate");
      AccArgs A = group_acc_args(q, vc, op, ng, init);
      A.codes = kc.dict_codes.as<uint16_t>(); A.rank_of_code = rank.as<uint32_t>();
      launch_group_accumulate(s, GROUP_SRC_CODES, A, GroupAccExtra{});
    }
  } else ng = groupreduce_hashed(q, key_p, kc, vc, op, nsel, init, T);
  launch_group_finish(s, q->gr_val.as<uint64_t>(), ng, kinds[0], op);
  stream_wait(ctx);                                        // the tables die here
  { RecycleScope rs; T = UniqueTables(); }
  q->gr_n = ng; q->gr_state = 2;
  if (ngroups) *ngroups = ng;
  if (key_bytes && dt_base(kc.dtype) == DFDB_STRING) *key_bytes = query_string_bytes(q, key_p);
}

// the counts of `ng` groups and the accumulators of `nvals` reducers (reducer-major) off the device; the counts to the caller's buffer as well
static void fetch_group_results(dfdb_query* q, int64_t ng, int nvals, std::vector<uint64_t>& c, std::vector<uint64_t>& v, int64_t* counts) {
  dfdb_ctx* ctx = q->t->ctx; hipStream_t s = ctx->stream;
  c.resize((size_t)ng); v.resize((size_t)ng * (size_t)nvals);
  HIP_CHECK(hipMemcpyAsync(c.data(), q->gr_cnt.p, (size_t)ng * 8, hipMemcpyDeviceToHost, s));
  if (nvals) HIP_CHECK(hipMemcpyAsync(v.data(), q->gr_val.p, v.size() * 8, hipMemcpyDeviceToHost, s));
  stream_wait(ctx);
  if (counts) memcpy(counts, c.data(), (size_t)ng * 8);
}
// the groups' keys (gathered over the first occurrences, i.e. in order of first appearance), counts and values -> caller buffers (host);
// restores the query's full selection afterwards
void query_groupreduce_fetch(dfdb_query* q, dfdb_outcol* keys, int64_t* counts, int64_t* vals_i, double* vals_f) {
  dfdb_table* t = q->t;
  if (q->gr_state == 0 || q->gr_multi == 2) fail(DFDB_ERR_ARGUMENT, "ArgumentError: dfdb_query_groupreduce has not been called (or the query was executed, reset or changed since)");
  if (q->bitmap_rows != t->nrows) { q->gr_state = 0; fail(DFDB_ERR_ARGUMENT, "ArgumentError: the table changed between dfdb_query_groupreduce and its fetch"); }
  const int64_t ng = q->gr_n;
  if (ng > 0) {
    if (keys) { keys->memkind = keys->memkind == DFDB_MEM_DEVICE ? DFDB_MEM_DEVICE : DFDB_MEM_HOST; materialize_col(q, q->gr_keys_n[0], *keys, ng); }
    std::vector<uint64_t> c, v;
    fetch_group_results(q, ng, 1, c, v, counts);
    group_values_out(v.data(), ng, q->gr_kinds_n.empty() ? 0 : q->gr_kinds_n[0], vals_i, vals_f);   // (no kind: an _n call without a reducer that was handed over)
  } else if (keys) { keys->count = 0; keys->nbytes = 0; }
  if (q->gr_state == 2) restore_group_selection(q);      // back to the full selection: bitmap + tile counts + prefix
  q->gr_state = 0;
}

// ---- groupreduce by a tuple of key columns with several reducers (dfdb_query_groupreduce_n; aggregate.jl:1-14 takes `by::Tuple{Vararg{Symbol}}` and any number of
// `name = col => Stat()`).  One group per distinct tuple (isequal, element by element), groups in order of the first selected row that holds the tuple.
// Device side, per call: G (4 bytes per row) and image (8 bytes per row) from the buffer pool —
//   rank    per key column, unique's forms over the full selection (the table complete and verified: no deferred verify, no optimistic prefix, no head-only dense
//           table, no radix form) and k_group_rank: the rank r_i of every selected row's key -> G for the first key, image = G * n_i + r_i for every later one;
//   fold    the image is ranked again, as a transient UInt64 column, into G: the first appearance of image is the first appearance of the tuple so far.  The last
//           ranking leaves q's bitmap narrowed to the groups' first rows — what the fetch gathers the keys from;
//   reduce  one pass for the count and every reducer (k_group_acc_multi), launch_group_finish per reducer at the end.
// A column that has no room for its scratch is DFDB_ERR_NOMEM, never a wrong answer.
struct PooledColumn {                                          // a transient column over pooled memory: back to the pool when the call ends, the stream drained first
  dfdb_ctx* ctx; Column col;
  explicit PooledColumn(dfdb_ctx* c) : ctx(c) {}
  ~PooledColumn() { (void)hipStreamSynchronize(ctx->stream); RecycleScope rs; col.data.release(); }
};
static uint64_t read_flag(dfdb_ctx* ctx, const DevBuf& flag) {
  uint64_t f = 0;
  HIP_CHECK(hipMemcpyAsync(&f, flag.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  stream_wait(ctx);
  return f;
}
// the rank of every selected row's key in column kc (q's bitmap holds the full selection, gr_sel a copy of it) -> g_out, or the image gprev * n + rank -> img_out;
// q's bitmap narrowed to the key's first occurrences on return.  Returns n, the key's distinct values
static int64_t group_rank_key(dfdb_query* q, const Column& kc, const uint32_t* gprev, uint32_t* g_out, uint64_t* img_out, DevBuf& flag) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  RankArgs A{};
  A.sel = q->gr_sel.as<uint64_t>(); A.nrows = t->nrows; A.gprev = gprev; A.g_out = g_out; A.img_out = img_out; A.flag = flag.as<uint64_t>();
  HIP_CHECK(hipMemsetAsync(flag.p, 0, 8, s));
  int64_t n = 0;
  bool ok;
  if (kc.dict_n > 0) {                                         // K9: the dictionary codes' ranks, no table
    n = dict_unique(q, kc, &q->du_rank);
    A.codes = kc.dict_codes.as<uint16_t>(); A.rank_of_code = q->du_rank.as<uint32_t>(); A.n = (uint64_t)n;
    LaunchTimer lt(ctx, "group_rank");
    ok = launch_group_rank(s, 1, A);
  } else {
    UniqueTables T;
    UniqueRequest R;                                            // a complete, verified table ...
    R.allow_radix = false;                                      // ... and a table it must be
    unique_impl_col(q, kc, R, &T);
    n = query_count(q, -1);
    A.n = (uint64_t)n; A.special = T.ctl()->head.special_row;
    const ColRef key = col_ref(kc);
    A.keycol = key.data; A.keydt = key.dtype; A.missing = T.is_str ? nullptr : key.missing;
    LaunchTimer lt(ctx, "group_rank");
    if (T.dense) {
      launch_dense_group_ids(s, T.first.as<uint64_t>(), T.range, T.ctl(), q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>());
      A.lo = T.lo; A.range = T.range; A.gids = T.first.as<uint64_t>();
      if (T.span_lo <= T.span_hi && T.span_hi < (uint64_t)T.range) {      // the table is laid out wider than the keys: only the span they cover (small: in LDS)
        A.lo = T.lo + T.span_lo; A.range = (uint32_t)(T.span_hi - T.span_lo + 1); A.gids = T.first.as<uint64_t>() + T.span_lo;
      }
      ok = launch_group_rank(s, 2, A);
    } else {
      launch_group_ids(s, T.ent.as<UniqueEntry>(), T.cap, T.ctl()->head.special_row, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>());
      A.ent = T.ent.as<UniqueEntry>(); A.mask = T.cap - 1;
      if (T.is_str) ok = launch_group_rank_str(s, A, str_side(kc), T.salt);
      else ok = launch_group_rank(s, 0, A);
    }
    stream_wait(ctx);                                          // the tables die here
    { RecycleScope rs; T = UniqueTables(); }
  }
  if (!ok) fail(DFDB_ERR_DEVICE, "groupreduce: the rank pass could not be launched");
  if (read_flag(ctx, flag)) fail(DFDB_ERR_DEVICE, "groupreduce: a selected row's key has no rank among %lld distinct values", (long long)n);
  return n;
}

void query_groupreduce_n(dfdb_query* q, const int32_t* key_cols, int32_t nkeys, const int32_t* val_cols, const int32_t* stats, int32_t nvals, int64_t* ngroups,
                         int64_t* key_bytes) {
  ensure_executed_checked(q);
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const std::vector<int> kinds = groupreduce_check(q, key_cols, nkeys, val_cols, stats, nvals);
  // the shape that dfdb_query_groupreduce answers: handed to it (the same answers, bit for bit, at the same speed)
  if (nkeys == 1 && nvals <= 1) {
    query_groupreduce(q, key_cols[0], nvals ? val_cols[0] : -1, nvals ? stats[0] : DFDB_AGG_COUNT, ngroups, key_bytes);
    q->gr_multi = 1;
    q->gr_keys_n.assign(key_cols, key_cols + 1); q->gr_ops_n.assign(stats, stats + nvals); q->gr_kinds_n = kinds;
    return;
  }
  std::vector<const Column*> kcs((size_t)nkeys), vcs((size_t)nvals, nullptr);
  for (int k = 0; k < nkeys; k++) kcs[(size_t)k] = &need_resident(t, q->proj[(size_t)key_cols[k]].expr->col);
  for (int m = 0; m < nvals; m++) if (stats[m] != DFDB_AGG_COUNT) vcs[(size_t)m] = &need_resident(t, q->proj[(size_t)val_cols[m]].expr->col);
  q->gr_state = 0; q->gr_n = 0; q->gr_multi = 2;
  q->gr_keys_n.assign(key_cols, key_cols + nkeys); q->gr_ops_n.assign(stats, stats + nvals); q->gr_kinds_n = kinds;
  if (ngroups) *ngroups = 0;
  if (key_bytes) for (int k = 0; k < nkeys; k++) key_bytes[k] = 0;
  const int64_t nsel = query_count(q, -1);
  if (nsel == 0 || t->nrows == 0) { q->gr_state = 1; return; }
  if (t->nrows >= (1ll << 32)) fail(DFDB_ERR_UNSUPPORTED, "groupreduce by several keys: group numbers are 32-bit, the table has %lld rows", (long long)t->nrows);
  const size_t nw = padded_words(t->nrows);
  q->gr_sel.ensure(nw * 8);
  HIP_CHECK(hipMemcpyAsync(q->gr_sel.p, q->bitmap.p, nw * 8, hipMemcpyDeviceToDevice, s));
  PooledScratch gbuf(ctx), flag(ctx);
  PooledColumn image(ctx);
  image.col.dtype = DFDB_U64; image.col.resident = true; image.col.nrows = t->nrows; image.col.name = "(groupreduce image)";
  if (!try_ensure(gbuf.buf, (size_t)t->nrows * 4 + 256) || !try_ensure(flag.buf, 64) || (nkeys > 1 && !try_ensure(image.col.data, (size_t)t->nrows * 8 + 256)))
    fail(DFDB_ERR_NOMEM, "groupreduce: no room for the group numbers of %lld rows", (long long)t->nrows);
  uint32_t* G = gbuf.buf.as<uint32_t>();
  int64_t ng = group_rank_key(q, *kcs[0], nullptr, G, nullptr, flag.buf);
  for (int k = 1; k < nkeys; k++) {
    restore_group_selection(q);                               // (the rank pass narrowed the bitmap: the full selection again)
    (void)group_rank_key(q, *kcs[(size_t)k], G, nullptr, image.col.data.as<uint64_t>(), flag.buf);
    restore_group_selection(q);
    ng = group_rank_key(q, image.col, nullptr, G, nullptr, flag.buf);
  }
  // q's bitmap holds the groups' first rows (prefix scanned): G numbers them in that order
  q->gr_cnt.ensure((size_t)ng * 8 + 64); q->gr_val.ensure((size_t)std::max(nvals, 1) * (size_t)ng * 8 + 64);
  HIP_CHECK(hipMemsetAsync(q->gr_cnt.p, 0, (size_t)ng * 8 + 64, s));
  for (int m = 0; m < nvals; m++) HIP_CHECK(hipMemsetAsync(q->gr_val.as<uint64_t>() + (size_t)m * ng, stats[m] == DFDB_AGG_MIN ? 0xFF : 0, (size_t)ng * 8, s));
  MultiAccArgs A{};
  A.sel = q->gr_sel.as<uint64_t>(); A.gid = G; A.nrows = t->nrows; A.nvals = nvals;
  for (int m = 0; m < nvals; m++) { const ColRef v = col_ref(vcs[(size_t)m]); A.valcol[m] = v.data; A.valdt[m] = v.dtype; A.op[m] = stats[m]; A.kind[m] = kinds[(size_t)m]; }
  A.cnt = q->gr_cnt.as<uint64_t>(); A.val = q->gr_val.as<uint64_t>(); A.ngroups = ng; A.flag = flag.buf.as<uint64_t>();
  HIP_CHECK(hipMemsetAsync(flag.buf.p, 0, 8, s));
  int form;
  { LaunchTimer lt(ctx, "group_accumulate_multi"); form = launch_group_accumulate_multi(s, A); }
  if (form < 0) fail(DFDB_ERR_DEVICE, "groupreduce: the accumulate pass could not be launched");
  if (read_flag(ctx, flag.buf)) fail(DFDB_ERR_DEVICE, "groupreduce: a selected row has no group among %lld", (long long)ng);
  prof_note(ctx, form ? "group_accumulate_multi.lds" : "group_accumulate_multi.global");
  for (int m = 0; m < nvals; m++) launch_group_finish(s, q->gr_val.as<uint64_t>() + (size_t)m * ng, ng, kinds[(size_t)m], stats[m]);
  stream_wait(ctx);
  q->gr_n = ng; q->gr_state = 2;
  if (ngroups) *ngroups = ng;
  if (key_bytes) for (int k = 0; k < nkeys; k++) if (dt_base(kcs[(size_t)k]->dtype) == DFDB_STRING) key_bytes[k] = query_string_bytes(q, key_cols[k]);
}

// the groups' keys (one dfdb_outcol per key column, gathered over the first rows), counts and values (reducer-major; a count reducer's values are the counts)
// -> caller buffers (host); restores the query's full selection afterwards
void query_groupreduce_n_fetch(dfdb_query* q, dfdb_outcol* keys, int64_t* counts, int64_t* vals_i, double* vals_f) {
  dfdb_table* t = q->t;
  if (q->gr_state == 0 || q->gr_multi == 0) fail(DFDB_ERR_ARGUMENT, "ArgumentError: dfdb_query_groupreduce_n has not been called (or the query was executed, reset or changed since)");
  const int nvals = (int)q->gr_ops_n.size();
  if (q->gr_multi == 1) {                                      // handed to dfdb_query_groupreduce: its fetch, and a count reducer's values from the counts
    const int64_t ng = q->gr_n;
    std::vector<int64_t> c((size_t)std::max<int64_t>(ng, 1));
    const bool cnt_red = nvals == 1 && q->gr_ops_n[0] == DFDB_AGG_COUNT;
    query_groupreduce_fetch(q, keys, c.data(), nvals && !cnt_red ? vals_i : nullptr, nvals && !cnt_red ? vals_f : nullptr);
    if (counts && ng > 0) memcpy(counts, c.data(), (size_t)ng * 8);
    if (cnt_red) group_values_out((const uint64_t*)c.data(), ng, 0, vals_i, vals_f);
    q->gr_multi = 0;
    return;
  }
  if (q->bitmap_rows != t->nrows) { q->gr_state = 0; fail(DFDB_ERR_ARGUMENT, "ArgumentError: the table changed between dfdb_query_groupreduce_n and its fetch"); }
  const int64_t ng = q->gr_n;
  const int nkeys = (int)q->gr_keys_n.size();
  if (ng > 0) {
    if (keys) for (int k = 0; k < nkeys; k++) { keys[k].memkind = keys[k].memkind == DFDB_MEM_DEVICE ? DFDB_MEM_DEVICE : DFDB_MEM_HOST; materialize_col(q, q->gr_keys_n[(size_t)k], keys[k], ng); }
    std::vector<uint64_t> c, v;
    fetch_group_results(q, ng, nvals, c, v, counts);
    for (int m = 0; m < nvals; m++) {
      const bool cnt_red = q->gr_ops_n[(size_t)m] == DFDB_AGG_COUNT;
      const size_t m0 = (size_t)m * (size_t)ng;
      group_values_out(cnt_red ? c.data() : v.data() + m0, ng, cnt_red ? 0 : q->gr_kinds_n[(size_t)m], vals_i ? vals_i + m0 : nullptr, vals_f ? vals_f + m0 : nullptr);
    }
  } else if (keys) for (int k = 0; k < nkeys; k++) { keys[k].count = 0; keys[k].nbytes = 0; }
  if (q->gr_state == 2) restore_group_selection(q);      // back to the full selection: bitmap + tile counts + prefix
  q->gr_state = 0; q->gr_multi = 0;
}

}  // namespace dfdb
