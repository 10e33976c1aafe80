// join.cpp — two views related on one key: dfdb_query_join (everything up to the number of pairs) and dfdb_query_join_fetch (the two row lists), over the
// kernels of k_join.hip and the sorted pairs of sort.cpp.
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
