// join.cpp — two views related on one key: dfdb_query_join (everything up to the number of pairs) and dfdb_query_join_fetch (the two row lists), over the
// kernels of k_join.hip and the sorted pairs of sort.cpp; and on several keys, String keys among them: dfdb_query_join_n (query_join_n below: the right side
// ordered by the sort driver, one refinement stage per 8-byte sub-key), whose lists the same fetch writes.
//
// The reference has no join: "several tables with possibility of joins" stands on its roadmap (docs/src/index.md:598) and a user materializes both sides and
// merges them on the host.  The semantics are DataFrames.jl's innerjoin / leftjoin / semijoin / antijoin with matchmissing = :notequal, restated in
// include/dfdb.h.  The host side plans: the right side's selected, non-missing keys sorted (K12), the left side's selected rows laid ascending, one probe launch
// (lo, cnt and the pairs per 1024 left rows), one scan; the fetch is one expand launch.  Every row and every key stays on the device.
#include "engine.hpp"
#include "ooc.hpp"
#include "join_rule.hpp"
#include <algorithm>

namespace dfdb {

namespace {
// call 1's device memory that the fetch does not need: from the pool, back to it when the call ends (the stream drained first)
struct JoinScratch {
  dfdb_ctx* ctx;
  DevBuf rkeys, rrows, grp_total, scan_scratch, aux, stage;
  explicit JoinScratch(dfdb_ctx* c) : ctx(c) {}
  ~JoinScratch() {
    (void)hipStreamSynchronize(ctx->stream);
    RecycleScope rs;
    for (DevBuf* b : {&rkeys, &rrows, &grp_total, &scan_scratch, &aux, &stage}) b->release();
  }
};
const char* const kJoinOn = "joining on";
// a call 1 that does not reach its end leaves nothing behind
struct DropUnlessDone { dfdb_query* q; bool done = false; ~DropUnlessDone() { if (!done) query_join_drop(q); } };
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

void query_join(dfdb_query* left, int32_t left_col, dfdb_query* right, int32_t right_col, int32_t kind, int64_t* npairs, int64_t* info) {
  left->jn_pending = false;                                   // whatever happens next, the earlier join's lists are gone (their buffers are taken over below)
  DropUnlessDone guard{left};
  if (kind != DFDB_JOIN_INNER && kind != DFDB_JOIN_LEFT && kind != DFDB_JOIN_SEMI && kind != DFDB_JOIN_ANTI)
    fail(DFDB_ERR_ARGUMENT, "ArgumentError: join kind %d (DFDB_JOIN_INNER, _LEFT, _SEMI or _ANTI)", kind);
  if (left->t->ctx != right->t->ctx) fail(DFDB_ERR_ARGUMENT, "ArgumentError: the two views of a join belong to different contexts");
  // every refusal before the first launch
  const Column& lc = ordered_column(left, left_col, kJoinOn);
  const Column& rc = ordered_column(right, right_col, kJoinOn);
  if (dt_base(lc.dtype) != dt_base(rc.dtype))
    fail(DFDB_ERR_UNSUPPORTED, "joining on columns of different types (%s and %s) is not supported: convert one side first", dt_name(dt_base(lc.dtype)).c_str(),
         dt_name(dt_base(rc.dtype)).c_str());
  check_join_rows(left->t, "left"); check_join_rows(right->t, "right");
  dfdb_table* lt = left->t; dfdb_ctx* ctx = lt->ctx; hipStream_t s = ctx->stream;

  // 1. the right side: its selected, non-missing keys in ascending order, equal keys in ascending row order
  JoinScratch S(ctx);
  int64_t nr = 0, rmiss = 0, passes = 0;
  query_sorted_key_pairs(right, rc, S.rkeys, S.rrows, &nr, &rmiss, &passes);
  const int64_t rsel = query_count(right, -1);
  // 2. the left side: its selected rows, ascending
  ensure_executed_checked(left);
  const int64_t nl = query_count(left, -1);
  int64_t inf[5] = {nl, rsel, 0, rmiss, passes};
  const int64_t groups = ceil_div(nl, kTileRows);
  int64_t total = 0;
  if (nl > 0) {
    left->jn_order.ensure((size_t)nl * 4);
    { LaunchTimer lt_(ctx, "sort_rows");
      launch_sort_rows(s, left->bitmap.as<uint64_t>(), left->tile_counts.as<uint32_t>(), left->prefix.as<uint64_t>(), lt->nrows, left->jn_order.as<uint32_t>(), nl); }
    // 3. the probe: lo, cnt, the pairs per 1024 left rows, the missing left rows
    left->jn_lo.ensure((size_t)groups * kTileRows * 4); left->jn_cnt.ensure((size_t)groups * kTileRows * 4);
    left->jn_base.ensure((size_t)(groups + 8) * 8);
    S.grp_total.ensure((size_t)(groups + 8) * 4); S.scan_scratch.ensure(scan_counts_scratch_bytes(groups)); S.aux.ensure(64);
    HIP_CHECK(hipMemsetAsync(S.aux.p, 0, 16, s));             // word 0: the missing left rows (64 bits); word 1: the overflow flag
    JoinProbe P{};
    P.order = left->jn_order.as<uint32_t>(); P.nl = nl; P.nrows = lt->nrows;
    P.rkeys = S.rkeys.as<uint64_t>(); P.nr = (uint32_t)nr; P.steps = join_search_steps((uint64_t)nr); P.kind = kind;
    P.lo = left->jn_lo.as<uint32_t>(); P.cnt = left->jn_cnt.as<uint32_t>(); P.grp_total = S.grp_total.as<uint32_t>();
    P.nmiss = (unsigned long long*)S.aux.p; P.flag = S.aux.as<uint32_t>() + 2;
    { LaunchTimer lt_(ctx, "join_probe"); launch_join_probe(s, col_ref(lc), P); }
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
  // 5. what the fetch needs stays with the left query: the right rows in key order move over, the right keys go back to the pool with the scratch
  {
    (void)hipStreamSynchronize(s);
    RecycleScope rs;
    left->jn_rrows = std::move(S.rrows);
  }
  left->jn_nl = nl; left->jn_npairs = total; left->jn_kind = kind; left->jn_lbase = lt->row_base; left->jn_rbase = right->t->row_base;
  left->jn_pending = true; guard.done = true;
  if (npairs) *npairs = total;
  if (info) memcpy(info, inf, sizeof inf);
}

// ---- the join on several keys, String keys among them (dfdb_query_join_n) ---------------------------------------------------------------------------
namespace {
// query_join_n's device memory that the fetch does not need; from the pool, back to it when the call ends (the stream drained first)
struct JoinNScratch {
  dfdb_ctx* ctx;
  SortOrderSink sorted;                                       // the right side's selected rows in tuple order, missing components included
  DevBuf rorder, rsub, rsub_rows, hist, tile_cnt, tile_base, grp_total, scan_scratch, aux;
  DevBuf row_off[DFDB_JOIN_MAX_KEYS];                         // a left String key's in-tile offsets (the right columns': the sort driver's own, in `sorted`)
  explicit JoinNScratch(dfdb_ctx* c) : ctx(c) {}
  ~JoinNScratch() {
    (void)hipStreamSynchronize(ctx->stream);
    RecycleScope rs;
    for (DevBuf* b : {&sorted.order, &rorder, &rsub, &rsub_rows, &hist, &tile_cnt, &tile_base, &grp_total, &scan_scratch, &aux}) b->release();
    for (DevBuf& b : row_off) b.release();
    for (DevBuf& b : sorted.row_off) b.release();
  }
};
// the profile's name of refinement stage 1, 2, .. beside the family's "join_refine" (the stages past the eighth share one)
const char* stage_name(int64_t stage) {
  static const char* const names[] = {"join_refine.1", "join_refine.2", "join_refine.3", "join_refine.4", "join_refine.5", "join_refine.6", "join_refine.7", "join_refine.8"};
  return stage >= 1 && stage <= 8 ? names[stage - 1] : "join_refine.9+";
}
// the nullable ones of a side's key columns, as the live walk reads them
JoinKeyMiss key_miss(const Column* const* cols, int32_t nkeys) {
  JoinKeyMiss K{};
  for (int32_t j = 0; j < nkeys; j++) {
    const Column& c = *cols[j];
    if (!dt_nullable(c.dtype)) continue;
    if (dt_base(c.dtype) == DFDB_STRING) K.sizes[K.n] = c.data.as<int32_t>(); else K.missing[K.n] = c.missing.as<uint64_t>();
    K.n++;
  }
  return K;
}
}  // namespace

// The plan: the right side's selected rows in tuple order by THE sort driver (a sink on it: no second driver), the rows with a missing
// component dropped from that order by a stable compaction -> rorder[0 .. nr), which becomes jn_rrows; the left side's selected rows laid ascending, every entry
// starting at the whole run (lo = 0, cnt = nr; an entry with a missing component: cnt = 0); then one refinement stage per 8-byte sub-key, the major key first
// — (a) rsub[i] = the sub-key of right row rorder[i], by the sort's own rekey / strkey write phase over rorder, (b) k_join_refine —; after the last stage the
// group totals are scanned and the total read back, as query_join does.  What is left pending in `left` is what query_join leaves: the fetch is the same
void query_join_n(dfdb_query* left, const int32_t* left_cols, dfdb_query* right, const int32_t* right_cols, int32_t nkeys, int32_t kind, int64_t* npairs, int64_t* info) {
  left->jn_pending = false;
  DropUnlessDone guard{left};
  if (kind != DFDB_JOIN_INNER && kind != DFDB_JOIN_LEFT && kind != DFDB_JOIN_SEMI && kind != DFDB_JOIN_ANTI)
    fail(DFDB_ERR_ARGUMENT, "ArgumentError: join kind %d (DFDB_JOIN_INNER, _LEFT, _SEMI or _ANTI)", kind);
  if (left->t->ctx != right->t->ctx) fail(DFDB_ERR_ARGUMENT, "ArgumentError: the two views of a join belong to different contexts");
  if (nkeys < 1 || nkeys > DFDB_JOIN_MAX_KEYS) fail(DFDB_ERR_ARGUMENT, "ArgumentError: %d join keys (1 to %d)", nkeys, (int)DFDB_JOIN_MAX_KEYS);
  if (!left_cols || !right_cols) fail(DFDB_ERR_ARGUMENT, "ArgumentError: no %s key columns", left_cols ? "right" : "left");
  // every refusal before the first launch
  const Column* lcs[DFDB_JOIN_MAX_KEYS]; const Column* rcs[DFDB_JOIN_MAX_KEYS];
  for (int32_t j = 0; j < nkeys; j++) {
    lcs[j] = &ordered_column(left, left_cols[j], kJoinOn, true);
    rcs[j] = &ordered_column(right, right_cols[j], kJoinOn, true);
    if (dt_base(lcs[j]->dtype) != dt_base(rcs[j]->dtype))
      fail(DFDB_ERR_UNSUPPORTED, "joining on columns of different types (key %d: %s and %s) is not supported: convert one side first", (int)j,
           dt_name(dt_base(lcs[j]->dtype)).c_str(), dt_name(dt_base(rcs[j]->dtype)).c_str());
  }
  check_join_rows(left->t, "left"); check_join_rows(right->t, "right");
  dfdb_table* lt = left->t; dfdb_table* rt = right->t; dfdb_ctx* ctx = lt->ctx; hipStream_t s = ctx->stream;

  // 1. the right side: the sort driver's order of its selected rows, then without the rows that have a missing component
  JoinNScratch S(ctx);
  {
    int32_t flags[DFDB_JOIN_MAX_KEYS] = {};
    query_sort_indices_n(right, right_cols, flags, nkeys, -1, nullptr, 0, DFDB_MEM_DEVICE, nullptr, nullptr, true, &S.sorted);
  }
  const int64_t rsel = S.sorted.n;
  int64_t nr = rsel;
  const JoinKeyMiss rmiss = key_miss(rcs, nkeys);
  if (rsel > 0 && rmiss.n > 0) {
    const int64_t rtiles = ceil_div(rsel, kTileRows);
    S.tile_cnt.ensure((size_t)(rtiles + 8) * 4); S.tile_base.ensure((size_t)(rtiles + 8) * 8); S.scan_scratch.ensure(scan_counts_scratch_bytes(rtiles));
    S.rorder.ensure((size_t)rsel * 4);
    JoinLive L{};
    L.order = S.sorted.order.as<uint32_t>(); L.n = rsel; L.nrows = rt->nrows; L.keys = rmiss;
    L.live_cnt = S.tile_cnt.as<uint32_t>(); L.live_base = S.tile_base.as<uint64_t>(); L.out = S.rorder.as<uint32_t>(); L.cap = rsel;
    { LaunchTimer lt_(ctx, "join_live"); launch_join_live(s, L, JOIN_LIVE_COUNT); }
    { LaunchTimer lt_(ctx, "scan_counts"); launch_scan_counts(s, L.live_cnt, S.tile_base.as<uint64_t>(), rtiles, S.scan_scratch.as<uint64_t>()); }
    { LaunchTimer lt_(ctx, "join_live"); launch_join_live(s, L, JOIN_LIVE_PLACE); }
    HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, S.tile_base.as<uint64_t>() + rtiles, 8, hipMemcpyDeviceToHost, s));
    stream_wait(ctx);
    nr = ctx->pinned_scalar[0];
  } else if (rsel > 0) {
    RecycleScope rs;
    S.rorder = std::move(S.sorted.order);                     // no component can be missing: the order is rorder
  }
  // 2. the left side: its selected rows, ascending
  ensure_executed_checked(left);
  const int64_t nl = query_count(left, -1);
  int64_t inf[6] = {nl, rsel, 0, rsel - nr, S.sorted.passes, 0};
  const int64_t groups = ceil_div(nl, kTileRows);
  int64_t total = 0;
  if (nl > 0) {
    left->jn_order.ensure((size_t)nl * 4);
    { LaunchTimer lt_(ctx, "sort_rows");
      launch_sort_rows(s, left->bitmap.as<uint64_t>(), left->tile_counts.as<uint32_t>(), left->prefix.as<uint64_t>(), lt->nrows, left->jn_order.as<uint32_t>(), nl); }
    left->jn_lo.ensure((size_t)groups * kTileRows * 4); left->jn_cnt.ensure((size_t)groups * kTileRows * 4);
    left->jn_base.ensure((size_t)(groups + 8) * 8);
    S.grp_total.ensure((size_t)(groups + 8) * 4); S.scan_scratch.ensure(scan_counts_scratch_bytes(groups)); S.aux.ensure(64);
    HIP_CHECK(hipMemsetAsync(S.aux.p, 0, 16, s));             // word 0: the left rows with a missing component (64 bits); word 1: the overflow flag
    JoinLive L{};
    L.order = left->jn_order.as<uint32_t>(); L.n = nl; L.nrows = lt->nrows; L.keys = key_miss(lcs, nkeys);
    L.lo = left->jn_lo.as<uint32_t>(); L.cnt = left->jn_cnt.as<uint32_t>(); L.nr = (uint32_t)nr; L.nmiss = (unsigned long long*)S.aux.p;
    // 3. the stages: the sub-keys of the key tuple, the major key first; a String key: chunk 0 .. m - 1, then the length
    int64_t nsub = 0;
    if (nr > 0) for (int32_t j = 0; j < nkeys; j++) nsub += dt_base(rcs[j]->dtype) == DFDB_STRING ? S.sorted.str_chunks[j] + 1 : 1;
    inf[5] = nsub;
    if (nsub == 0) { L.grp_total = S.grp_total.as<uint32_t>(); L.emit0 = (uint32_t)join_emitted(kind, 0); }     // no stage will run: every entry emits what cnt = 0 emits
    { LaunchTimer lt_(ctx, "join_live"); launch_join_live(s, L, JOIN_LIVE_START); }
    if (nsub > 0) {
      S.rsub.ensure((size_t)nr * 8); S.rsub_rows.ensure((size_t)nr * 4); S.hist.ensure((size_t)(kSelectMaxRanks * 256 + 8) * 8);
      HIP_CHECK(hipMemsetAsync(S.hist.p, 0, (size_t)(8 * 256 + 1) * 8, s));       // (the write phase counts its key bytes with its LDS histograms and global atomics: nobody reads them here — a follow-up)
    }
    JoinRefine P{};
    P.order = left->jn_order.as<uint32_t>(); P.nl = nl; P.nrows = lt->nrows; P.rsub = S.rsub.as<uint64_t>();
    P.lo = left->jn_lo.as<uint32_t>(); P.cnt = left->jn_cnt.as<uint32_t>(); P.kind = kind;
    P.grp_total = S.grp_total.as<uint32_t>(); P.flag = S.aux.as<uint32_t>() + 2;
    int64_t stage = 0;
    for (int32_t j = 0; j < nkeys && nsub > 0; j++) {
      const Column& lc = *lcs[j]; const Column& rc = *rcs[j];
      if (dt_base(rc.dtype) != DFDB_STRING) {
        SortRekey R{};                                        // (a) no live base and no entry missing: sub-key i lands at i
        R.order = S.rorder.as<uint32_t>(); R.n = nr; R.nrows = rt->nrows; R.flip = 0;
        R.keys = S.rsub.as<uint64_t>(); R.rows = S.rsub_rows.as<uint32_t>(); R.cap = nr; R.ghist = (unsigned long long*)S.hist.p;
        { LaunchTimer lt_(ctx, "sort_rekey"); launch_sort_rekey(s, col_ref(rc), R, false); }
        P.last = ++stage == nsub;
        { LaunchTimer lt_(ctx, "join_refine"); LaunchTimer st_(ctx, stage_name(stage)); launch_join_refine(s, col_ref(lc), P); }
        continue;
      }
      const int64_t m = S.sorted.str_chunks[j];
      // the in-tile offsets a chunk needs (m > 0): the right column's are the ones the sort driver built; the left column's are built once per COLUMN
      int32_t lo_at = j;
      for (int32_t i = 0; i < j; i++) if (lcs[i] == lcs[j] && S.row_off[i].p) { lo_at = i; break; }
      if (m > 0 && lo_at == j) {
        S.row_off[j].ensure((size_t)std::max<int64_t>(lt->nrows, 1) * 4);
        LaunchTimer lt_(ctx, "str_row_offsets"); launch_str_row_offsets(s, lc.data.as<int32_t>(), S.row_off[j].as<uint32_t>(), lt->nrows);
      }
      const uint32_t* lrow_off = S.row_off[lo_at].as<uint32_t>();
      const uint32_t* rrow_off = S.sorted.row_off[j].as<uint32_t>();
      for (int64_t k = 0; k <= m; k++) {
        const int32_t chunk = k < m ? (int32_t)k : -1;
        SortStrKey R{};
        R.order = S.rorder.as<uint32_t>(); R.n = nr; R.nrows = rt->nrows; R.flip = 0; R.chunk = chunk;
        R.keys = S.rsub.as<uint64_t>(); R.rows = S.rsub_rows.as<uint32_t>(); R.cap = nr; R.ghist = (unsigned long long*)S.hist.p;
        { LaunchTimer lt_(ctx, chunk < 0 ? "sort_strkey_len" : "sort_strkey"); launch_sort_strkey(s, str_side(rc), rrow_off, R, false); }
        P.last = ++stage == nsub;
        { LaunchTimer lt_(ctx, "join_refine"); LaunchTimer st_(ctx, stage_name(stage)); launch_join_refine_str(s, JoinStrSub{str_side(lc), lrow_off, chunk}, P); }
      }
    }
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
  // 5. what the fetch needs stays with the left query: the right rows in tuple order move over
  {
    (void)hipStreamSynchronize(s);
    RecycleScope rs;
    left->jn_rrows = std::move(S.rorder);
  }
  left->jn_nl = nl; left->jn_npairs = total; left->jn_kind = kind; left->jn_lbase = lt->row_base; left->jn_rbase = rt->row_base;
  left->jn_pending = true; guard.done = true;
  if (npairs) *npairs = total;
  if (info) memcpy(info, inf, sizeof inf);
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
