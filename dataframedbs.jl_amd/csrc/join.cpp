// join.cpp — two views related on their keys: call 1 (everything up to the number of pairs: dfdb_query_join on one fixed-width key, dfdb_query_join_n on one
// to eight keys, String keys among them) and dfdb_query_join_fetch (the two row lists), over the kernels of k_join.hip and the sort driver of sort.cpp.
//
// The reference has no join: "several tables with possibility of joins" stands on its roadmap (docs/src/index.md:598) and a user materializes both sides and
// merges them on the host.  The semantics are DataFrames.jl's innerjoin / leftjoin / semijoin / antijoin with matchmissing = :notequal, restated in
// include/dfdb.h.  Every row and every key stays on the device.
//
// ONE driver (join_call) is call 1 of both entry points: the refusals, the right side in key order, the left side's selected rows laid ascending, a match step
// that leaves per left entry its run of the right order (lo, cnt) and per 1024 entries their pairs, one scan of those totals, the hand-over to the fetch.
// Only the match step — and the right side it searches — differs, in two PLANS, chosen by the entry point and not by the keys:
//   PROBE  (dfdb_query_join)    the right side's non-missing {key, row} pairs sorted (query_sorted_key_pairs), one probe launch: two searches per left entry
//   REFINE (dfdb_query_join_n)  the right side's rows in tuple order by THE sort driver (a sink on it), the rows with a missing component dropped from that
//                               order; every left entry starts at the whole run and one refinement stage per 8-byte sub-key narrows it
// The fetch is one expand launch, whichever plan ran.
#include "engine.hpp"
#include "ooc.hpp"
#include "join_rule.hpp"
#include <algorithm>

namespace dfdb {

namespace {
enum class JoinPlan { Probe, Refine };
// a call's device memory that does not stay with the left query: from the pool, back to it when the call ends (the stream drained first)
struct JoinScratch {
  dfdb_ctx* ctx;
  DevBuf rrows;                                               // the right side's live rows in key order: what becomes jn_rrows
  DevBuf grp_total, scan_scratch, aux;                        // aux: the left rows with a missing component (64 bits), then the overflow flag
  DevBuf rkeys;                                               // PROBE: the sorted keys beside rrows
  SortOrderSink sorted;                                       // REFINE: the right side's selected rows in tuple order, missing components included
  DevBuf tile_cnt, tile_base, rsub, rsub_rows, hist;          // REFINE: the live walk's counts; a stage's right sub-keys
  DevBuf row_off[DFDB_JOIN_MAX_KEYS];                         // REFINE: a left String key's in-tile offsets (the right columns': the sort driver's own, in `sorted`)
  DevBuf stage;                                               // the fetch: host outputs pass through it
  explicit JoinScratch(dfdb_ctx* c) : ctx(c) {}
  ~JoinScratch() {
    (void)hipStreamSynchronize(ctx->stream);
    RecycleScope rs;
    for (DevBuf* b : {&rrows, &grp_total, &scan_scratch, &aux, &rkeys, &sorted.order, &tile_cnt, &tile_base, &rsub, &rsub_rows, &hist, &stage}) b->release();
    for (DevBuf& b : row_off) b.release();
    for (DevBuf& b : sorted.row_off) b.release();
  }
};
// a call 1 that does not reach its end leaves nothing behind
struct DropUnlessDone { dfdb_query* q; bool done = false; ~DropUnlessDone() { if (!done) query_join_drop(q); } };
struct JoinKeys { const Column* l[DFDB_JOIN_MAX_KEYS]; const Column* r[DFDB_JOIN_MAX_KEYS]; };
}  // namespace

void query_join_drop(dfdb_query* q) {
  q->jn_pending = false;
  bool any = false;
  for (DevBuf* b : {&q->jn_order, &q->jn_lo, &q->jn_cnt, &q->jn_base, &q->jn_rrows}) any = any || b->p;
  if (!any) return;
  if (q->t) (void)hipStreamSynchronize(q->t->ctx->stream); else (void)hipDeviceSynchronize();      // (a fetch into device memory may still read them)
  RecycleScope rs;
  for (DevBuf* b : {&q->jn_order, &q->jn_lo, &q->jn_cnt, &q->jn_base, &q->jn_rrows}) b->release();
}

static void check_join_rows(const dfdb_table* t, const char* side) {
  if (t->nrows >= (int64_t)1 << 31) fail(DFDB_ERR_UNSUPPORTED, "joining a table of 2^31 rows or more (the %s side) is not supported: the pairs carry rows in 32 bits", side);
}

// Every refusal of call 1, all of them before the first launch: the kind, the contexts, the key lists, then key by key the left column, the right column and
// their types, then the row counts.  strings: dfdb_query_join_n, which admits String keys and whose type mismatch names the key position
static JoinKeys check_join(dfdb_query* left, const int32_t* left_cols, dfdb_query* right, const int32_t* right_cols, int32_t nkeys, int32_t kind, bool strings) {
  if (kind != DFDB_JOIN_INNER && kind != DFDB_JOIN_LEFT && kind != DFDB_JOIN_SEMI && kind != DFDB_JOIN_ANTI)
    fail(DFDB_ERR_ARGUMENT, "ArgumentError: join kind %d (DFDB_JOIN_INNER, _LEFT, _SEMI or _ANTI)", kind);
  if (left->t->ctx != right->t->ctx) fail(DFDB_ERR_ARGUMENT, "ArgumentError: the two views of a join belong to different contexts");
  if (nkeys < 1 || nkeys > DFDB_JOIN_MAX_KEYS) fail(DFDB_ERR_ARGUMENT, "ArgumentError: %d join keys (1 to %d)", nkeys, (int)DFDB_JOIN_MAX_KEYS);
  if (!left_cols || !right_cols) fail(DFDB_ERR_ARGUMENT, "ArgumentError: no %s key columns", left_cols ? "right" : "left");
  JoinKeys K{};
  for (int32_t j = 0; j < nkeys; j++) {
    K.l[j] = &ordered_column(left, left_cols[j], "joining on", strings);
    K.r[j] = &ordered_column(right, right_cols[j], "joining on", strings);
    if (dt_base(K.l[j]->dtype) == dt_base(K.r[j]->dtype)) continue;
    const std::string where = strings ? "key " + std::to_string(j) + ": " : "";
    fail(DFDB_ERR_UNSUPPORTED, "joining on columns of different types (%s%s and %s) is not supported: convert one side first", where.c_str(),
         dt_name(dt_base(K.l[j]->dtype)).c_str(), dt_name(dt_base(K.r[j]->dtype)).c_str());
  }
  check_join_rows(left->t, "left"); check_join_rows(right->t, "right");
  return K;
}

// ---- the PROBE plan ------------------------------------------------------------------------------------------------------------------------------------
// the right side: its selected, non-missing keys in ascending order, equal keys in ascending row order.  Returns nr, the pairs; inf[1], [3], [4] are written
static int64_t probe_right_side(dfdb_query* right, const Column& rc, JoinScratch& S, int64_t* inf) {
  int64_t nr = 0;
  query_sorted_key_pairs(right, rc, S.rkeys, S.rrows, &nr, &inf[3], &inf[4]);
  inf[1] = query_count(right, -1);
  return nr;
}
// the match: lo, cnt, the pairs per 1024 left rows, the missing left rows
static void probe_match(dfdb_query* left, const Column& lc, JoinScratch& S, int64_t nl, int64_t nr, int32_t kind) {
  dfdb_ctx* ctx = left->t->ctx;
  JoinProbe P{};
  P.order = left->jn_order.as<uint32_t>(); P.nl = nl; P.nrows = left->t->nrows;
  P.rkeys = S.rkeys.as<uint64_t>(); P.nr = (uint32_t)nr; P.steps = join_search_steps((uint64_t)nr); P.kind = kind;
  P.lo = left->jn_lo.as<uint32_t>(); P.cnt = left->jn_cnt.as<uint32_t>(); P.grp_total = S.grp_total.as<uint32_t>();
  P.nmiss = (unsigned long long*)S.aux.p; P.flag = S.aux.as<uint32_t>() + 2;
  LaunchTimer lt_(ctx, "join_probe"); launch_join_probe(ctx->stream, col_ref(lc), P);
}

// ---- the REFINE plan -----------------------------------------------------------------------------------------------------------------------------------
// the profile's name of refinement stage 1, 2, .. beside the family's "join_refine" (the stages past the eighth share one)
static const char* stage_name(int64_t stage) {
  static const char* const names[] = {"join_refine.1", "join_refine.2", "join_refine.3", "join_refine.4", "join_refine.5", "join_refine.6", "join_refine.7", "join_refine.8"};
  return stage >= 1 && stage <= 8 ? names[stage - 1] : "join_refine.9+";
}
// the nullable ones of a side's key columns, as the live walk reads them
static JoinKeyMiss key_miss(const Column* const* cols, int32_t nkeys) {
  JoinKeyMiss K{};
  for (int32_t j = 0; j < nkeys; j++) {
    const Column& c = *cols[j];
    if (!dt_nullable(c.dtype)) continue;
    if (dt_base(c.dtype) == DFDB_STRING) K.sizes[K.n] = c.data.as<int32_t>(); else K.missing[K.n] = c.missing.as<uint64_t>();
    K.n++;
  }
  return K;
}
// the right side: the sort driver's order of its selected rows, then without the rows that have a missing component (a stable compaction) -> S.rrows[0 .. nr).
// Returns nr; inf[1], [3], [4] are written
static int64_t refine_right_side(dfdb_query* right, const int32_t* right_cols, const Column* const* rcs, int32_t nkeys, JoinScratch& S, int64_t* inf) {
  dfdb_ctx* ctx = right->t->ctx; hipStream_t s = ctx->stream;
  const int32_t flags[DFDB_JOIN_MAX_KEYS] = {};
  query_sort_indices_n(right, right_cols, flags, nkeys, -1, nullptr, 0, DFDB_MEM_DEVICE, nullptr, nullptr, true, &S.sorted);
  const int64_t rsel = S.sorted.n;
  int64_t nr = rsel;
  const JoinKeyMiss rmiss = key_miss(rcs, nkeys);
  if (rsel > 0 && rmiss.n > 0) {
    const int64_t rtiles = ceil_div(rsel, kTileRows);
    S.tile_cnt.ensure((size_t)(rtiles + 8) * 4); S.tile_base.ensure((size_t)(rtiles + 8) * 8); S.scan_scratch.ensure(scan_counts_scratch_bytes(rtiles));
    S.rrows.ensure((size_t)rsel * 4);
    JoinLive L{};
    L.order = S.sorted.order.as<uint32_t>(); L.n = rsel; L.nrows = right->t->nrows; L.keys = rmiss;
    L.live_cnt = S.tile_cnt.as<uint32_t>(); L.live_base = S.tile_base.as<uint64_t>(); L.out = S.rrows.as<uint32_t>(); L.cap = rsel;
    { LaunchTimer lt_(ctx, "join_live"); launch_join_live(s, L, JOIN_LIVE_COUNT); }
    { LaunchTimer lt_(ctx, "scan_counts"); launch_scan_counts(s, L.live_cnt, S.tile_base.as<uint64_t>(), rtiles, S.scan_scratch.as<uint64_t>()); }
    { LaunchTimer lt_(ctx, "join_live"); launch_join_live(s, L, JOIN_LIVE_PLACE); }
    HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, S.tile_base.as<uint64_t>() + rtiles, 8, hipMemcpyDeviceToHost, s));
    stream_wait(ctx);
    nr = ctx->pinned_scalar[0];
  } else if (rsel > 0) {
    RecycleScope rs;
    S.rrows = std::move(S.sorted.order);                      // no component can be missing: the order is the live order
  }
  inf[1] = rsel; inf[3] = rsel - nr; inf[4] = S.sorted.passes;
  return nr;
}
// the match: every entry starts at the whole run (lo = 0, cnt = nr; an entry with a missing component: cnt = 0), then one stage per 8-byte sub-key of the key
// tuple, the major key first; a String key: chunk 0 .. m - 1, then the length.  Returns the stages run
static int64_t refine_match(dfdb_query* left, const JoinKeys& K, int32_t nkeys, dfdb_table* rt, JoinScratch& S, int64_t nl, int64_t nr, int32_t kind) {
  dfdb_table* lt = left->t; dfdb_ctx* ctx = lt->ctx; hipStream_t s = ctx->stream;
  JoinLive L{};
  L.order = left->jn_order.as<uint32_t>(); L.n = nl; L.nrows = lt->nrows; L.keys = key_miss(K.l, nkeys);
  L.lo = left->jn_lo.as<uint32_t>(); L.cnt = left->jn_cnt.as<uint32_t>(); L.nr = (uint32_t)nr; L.nmiss = (unsigned long long*)S.aux.p;
  int64_t nsub = 0;
  if (nr > 0) for (int32_t j = 0; j < nkeys; j++) nsub += dt_base(K.r[j]->dtype) == DFDB_STRING ? S.sorted.str_chunks[j] + 1 : 1;
  if (nsub == 0) { L.grp_total = S.grp_total.as<uint32_t>(); L.emit0 = (uint32_t)join_emitted(kind, 0); }     // no stage will run: every entry emits what cnt = 0 emits
  { LaunchTimer lt_(ctx, "join_live"); launch_join_live(s, L, JOIN_LIVE_START); }
  if (nsub == 0) return 0;
  S.rsub.ensure((size_t)nr * 8); S.rsub_rows.ensure((size_t)nr * 4); S.hist.ensure((size_t)(kSelectMaxRanks * 256 + 8) * 8);
  HIP_CHECK(hipMemsetAsync(S.hist.p, 0, (size_t)(8 * 256 + 1) * 8, s));         // (the write phase counts its key bytes with its LDS histograms and global atomics: nobody reads them here — a follow-up)
  JoinRefine P{};
  P.order = left->jn_order.as<uint32_t>(); P.nl = nl; P.nrows = lt->nrows; P.rsub = S.rsub.as<uint64_t>();
  P.lo = left->jn_lo.as<uint32_t>(); P.cnt = left->jn_cnt.as<uint32_t>(); P.kind = kind;
  P.grp_total = S.grp_total.as<uint32_t>(); P.flag = S.aux.as<uint32_t>() + 2;
  // One stage: (a) rsub[i] = the sub-key of right row rrows[i], by the sort's own rekey / strkey write phase over rrows — no live base and no entry missing:
  // sub-key i lands at i —, (b) the refine.  R: the write phase's record (SortRekey / SortStrKey), what the two have in common filled here
  int64_t stage = 0;
  auto run_stage = [&](const char* write_name, auto R, auto&& write, auto&& refine) {
    R.order = S.rrows.as<uint32_t>(); R.n = nr; R.nrows = rt->nrows; R.flip = 0;
    R.keys = S.rsub.as<uint64_t>(); R.rows = S.rsub_rows.as<uint32_t>(); R.cap = nr; R.ghist = (unsigned long long*)S.hist.p;
    { LaunchTimer lt_(ctx, write_name); write(R); }
    P.last = ++stage == nsub;
    { LaunchTimer lt_(ctx, "join_refine"); LaunchTimer st_(ctx, stage_name(stage)); refine(); }
  };
  for (int32_t j = 0; j < nkeys; j++) {
    const Column& lc = *K.l[j]; const Column& rc = *K.r[j];
    if (dt_base(rc.dtype) != DFDB_STRING) {
      run_stage("sort_rekey", SortRekey{}, [&](const SortRekey& R) { launch_sort_rekey(s, col_ref(rc), R, false); }, [&] { launch_join_refine(s, col_ref(lc), P); });
      continue;
    }
    const int64_t m = S.sorted.str_chunks[j];
    // the in-tile offsets a chunk needs (m > 0): the right column's are the ones the sort driver built; the left column's are built once per COLUMN
    int32_t lo_at = j;
    for (int32_t i = 0; i < j; i++) if (K.l[i] == K.l[j] && S.row_off[i].p) { lo_at = i; break; }
    if (m > 0 && lo_at == j) {
      S.row_off[j].ensure((size_t)std::max<int64_t>(lt->nrows, 1) * 4);
      LaunchTimer lt_(ctx, "str_row_offsets"); launch_str_row_offsets(s, lc.data.as<int32_t>(), S.row_off[j].as<uint32_t>(), lt->nrows);
    }
    const uint32_t* lrow_off = S.row_off[lo_at].as<uint32_t>();
    const uint32_t* rrow_off = S.sorted.row_off[j].as<uint32_t>();
    for (int64_t k = 0; k <= m; k++) {
      SortStrKey R{};
      R.chunk = k < m ? (int32_t)k : -1;
      run_stage(R.chunk < 0 ? "sort_strkey_len" : "sort_strkey", R, [&](const SortStrKey& W) { launch_sort_strkey(s, str_side(rc), rrow_off, W, false); },
                [&] { launch_join_refine_str(s, JoinStrSub{str_side(lc), lrow_off, R.chunk}, P); });
    }
  }
  return nsub;
}

// ---- the driver ----------------------------------------------------------------------------------------------------------------------------------------
// Call 1.  ninfo: the words of `info` the entry point's caller holds (5: dfdb_query_join; 6: dfdb_query_join_n, the sixth being the stages run)
static void join_call(dfdb_query* left, const int32_t* left_cols, dfdb_query* right, const int32_t* right_cols, int32_t nkeys, int32_t kind, JoinPlan plan,
                      int64_t* npairs, int64_t* info, int ninfo) {
  left->jn_pending = false;                                   // whatever happens next, the earlier join's lists are gone (their buffers are taken over below)
  DropUnlessDone guard{left};
  const bool refine = plan == JoinPlan::Refine;
  const JoinKeys K = check_join(left, left_cols, right, right_cols, nkeys, kind, refine);
  dfdb_table* lt = left->t; dfdb_table* rt = right->t; dfdb_ctx* ctx = lt->ctx; hipStream_t s = ctx->stream;
  JoinScratch S(ctx);
  int64_t inf[6] = {};                                        // selected left rows, selected right rows, left / right rows that match nothing (missing), right passes, stages
  // 1. the right side in key order — before the left query is executed: the two may be one query
  const int64_t nr = refine ? refine_right_side(right, right_cols, K.r, nkeys, S, inf) : probe_right_side(right, *K.r[0], S, inf);
  // 2. the left side: its selected rows, ascending, and the arrays the match step fills
  ensure_executed_checked(left);
  const int64_t nl = inf[0] = query_count(left, -1);
  const int64_t groups = ceil_div(nl, kTileRows);
  int64_t total = 0;
  if (nl > 0) {
    left->jn_order.ensure((size_t)nl * 4);
    { LaunchTimer lt_(ctx, "sort_rows");
      launch_sort_rows(s, left->bitmap.as<uint64_t>(), left->tile_counts.as<uint32_t>(), left->prefix.as<uint64_t>(), lt->nrows, left->jn_order.as<uint32_t>(), nl); }
    left->jn_lo.ensure((size_t)groups * kTileRows * 4); left->jn_cnt.ensure((size_t)groups * kTileRows * 4);
    left->jn_base.ensure((size_t)(groups + 8) * 8);
    S.grp_total.ensure((size_t)(groups + 8) * 4); S.scan_scratch.ensure(scan_counts_scratch_bytes(groups)); S.aux.ensure(64);
    HIP_CHECK(hipMemsetAsync(S.aux.p, 0, 16, s));
    // 3. the match
    if (refine) inf[5] = refine_match(left, K, nkeys, rt, S, nl, nr, kind); else probe_match(left, *K.l[0], S, nl, nr, kind);
    // 4. where every group's pairs start; the total, the flag and the missing count in one wait
    { LaunchTimer lt_(ctx, "scan_counts");
      launch_scan_counts(s, S.grp_total.as<uint32_t>(), left->jn_base.as<uint64_t>(), groups, S.scan_scratch.as<uint64_t>()); }
    HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, left->jn_base.as<uint64_t>() + groups, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar + 1, S.aux.p, 16, hipMemcpyDeviceToHost, s));
    stream_wait(ctx);
    total = ctx->pinned_scalar[0]; inf[2] = ctx->pinned_scalar[1];
    if ((uint32_t)ctx->pinned_scalar[2] != 0)
      fail(DFDB_ERR_UNSUPPORTED, "a join with more than 2^32 - 1 pairs from 1024 consecutive left rows is not supported (the pairs of 1024 left rows are counted in 32 bits)");
  }
  // 5. what the fetch needs stays with the left query: the right rows in key order move over, everything else goes back to the pool with the scratch
  {
    (void)hipStreamSynchronize(s);
    RecycleScope rs;
    left->jn_rrows = std::move(S.rrows);
  }
  left->jn_nl = nl; left->jn_npairs = total; left->jn_kind = kind; left->jn_lbase = lt->row_base; left->jn_rbase = rt->row_base;
  left->jn_pending = true; guard.done = true;
  if (npairs) *npairs = total;
  if (info) memcpy(info, inf, (size_t)ninfo * sizeof inf[0]);
}

void query_join(dfdb_query* left, int32_t left_col, dfdb_query* right, int32_t right_col, int32_t kind, int64_t* npairs, int64_t* info) {
  join_call(left, &left_col, right, &right_col, 1, kind, JoinPlan::Probe, npairs, info, 5);
}
// (one fixed-width key takes the stages too: which kernel serves it best is DESIGN.md section 10's open measurement, and changing JoinPlan here is all it takes)
void query_join_n(dfdb_query* left, const int32_t* left_cols, dfdb_query* right, const int32_t* right_cols, int32_t nkeys, int32_t kind, int64_t* npairs, int64_t* info) {
  join_call(left, left_cols, right, right_cols, nkeys, kind, JoinPlan::Refine, npairs, info, 6);
}

void query_join_fetch(dfdb_query* left, int64_t* left_rows, int64_t* right_rows, int64_t cap, int32_t memkind) {
  if (!left->jn_pending) fail(DFDB_ERR_ARGUMENT, "ArgumentError: dfdb_query_join has not been called (or the query was reset since)");
  const int64_t n = left->jn_npairs;
  if (cap < n) fail(DFDB_ERR_BOUNDS, "BoundsError: the join has %lld pairs, capacity is %lld", (long long)n, (long long)cap);
  if (n == 0) return;
  if (!left_rows) fail(DFDB_ERR_ARGUMENT, "ArgumentError: no output buffer");
  dfdb_ctx* ctx = left->t->ctx; hipStream_t s = ctx->stream;
  JoinScratch S(ctx);
  JoinExpand E{};
  E.order = left->jn_order.as<uint32_t>(); E.lo = left->jn_lo.as<uint32_t>(); E.cnt = left->jn_cnt.as<uint32_t>(); E.nl = left->jn_nl;
  E.out_base = left->jn_base.as<uint64_t>(); E.rrows = left->jn_rrows.as<uint32_t>(); E.kind = left->jn_kind;
  E.lbase = left->jn_lbase; E.rbase = left->jn_rbase; E.left_rows = left_rows; E.right_rows = right_rows; E.cap = n;
  const bool dev = memkind == DFDB_MEM_DEVICE;
  if (!dev) {                                                 // as the sort does: a pooled stage, then one copy per list
    S.stage.ensure((size_t)n * 8 * (right_rows ? 2 : 1));
    E.left_rows = S.stage.as<int64_t>(); E.right_rows = right_rows ? S.stage.as<int64_t>() + n : nullptr;
  }
  { LaunchTimer lt_(ctx, "join_expand"); launch_join_expand(s, E); }
  if (!dev) {
    HIP_CHECK(hipMemcpyAsync(left_rows, E.left_rows, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (right_rows) HIP_CHECK(hipMemcpyAsync(right_rows, E.right_rows, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    stream_wait(ctx);
  }
}

}  // namespace dfdb
