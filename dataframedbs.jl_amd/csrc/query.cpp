// query.cpp — DFView on the device: SelectionQueue composition, stage execution, count, indices,
// materialize, aggregates.
//
// Replaces (paths under /root/reference): SelectionQueue add/_new_queue src/tables/selection.jl:37-60,
// SelectionExecutor.apply :161-167 with its range :94-111 and predicate :133-157 stages, the block loop of
// src/io/blocksiterator.jl:98-145, nrow src/tables/view.jl:192-206, ProjectionExecutor.eval_on_range
// src/tables/projection.jl:128-154 and materialize src/tables/materialization.jl:27-52.
//
// The reference walks blocks serially and carries a per-stage `offset`; here every stage is ONE pass over
// the whole resident column range, the mask is a packed bitmap in HBM, and the cross-block offset becomes
// an exclusive scan of per-tile popcounts.  The selection is evaluated once (no count pre-pass, quirk Q8):
// dfdb_count reads the scan total, dfdb_materialize reuses the same bitmap.
#include "engine.hpp"
#include "ooc.hpp"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>

namespace dfdb {

// launchers living in k_interp.hip / k_strings.hip that take engine-level descriptions
void run_interp_predicate(dfdb_query* q, const Node& pred, bool and_existing);
void run_interp_project(dfdb_query* q, const Node& expr, void* dst, int64_t cap, uint8_t* missing_dst);
void run_str_parse(dfdb_query* q, const Node& expr, void* dst, int64_t cap);   // k_parse.hip

// ---------------------------------------------------------------- ranges
static int64_t range_len(int64_t a, int64_t s, int64_t b) {
  if (s > 0) return b < a ? 0 : (b - a) / s + 1;
  return b > a ? 0 : (a - b) / (-s) + 1;
}
int64_t Stage::first() const {
  if (kind == ST_RANGE) return n == 0 ? INT64_MAX : (step > 0 ? start : stop);
  return idx.empty() ? INT64_MAX : *std::min_element(idx.begin(), idx.end());
}
int64_t Stage::last() const {
  if (kind == ST_RANGE) return n == 0 ? INT64_MIN : (step > 0 ? stop : start);
  return idx.empty() ? INT64_MIN : *std::max_element(idx.begin(), idx.end());
}
int64_t Stage::elem(int64_t k) const {
  if (k < 1 || k > n) fail(DFDB_ERR_BOUNDS, "BoundsError: attempt to access %lld-element selection at index [%lld]", (long long)n, (long long)k);
  return kind == ST_RANGE ? start + (k - 1) * step : idx[(size_t)k - 1];
}
static void normalise(Stage& s) {
  if (s.kind == ST_RANGE) {
    if (s.step == 0) fail(DFDB_ERR_ARGUMENT, "ArgumentError: step cannot be zero");
    s.n = range_len(s.start, s.step, s.stop);
    if (s.n > 0) s.stop = s.start + (s.n - 1) * s.step;
  } else if (s.kind != ST_PRED) s.n = (int64_t)s.idx.size();
}

// add(q, elem) with _new_queue's rules (selection.jl:39-49)
void query_add_stage(dfdb_query* q, Stage&& ns) {
  normalise(ns);
  q->executed_stages = -1; q->count = -1; q->prefix_valid = false; q->gr_state = 0;
  Stage* last = q->stages.empty() ? nullptr : &q->stages.back();
  const bool new_is_range = ns.kind != ST_PRED;
  if (last && last->kind != ST_PRED && new_is_range) {   // range∘range collapses to old[elem] (:40)
    Stage r;
    if (last->kind == ST_INTEGER) {                       // Number indexing: only x[1]
      if (!(ns.kind == ST_INTEGER && ns.idx[0] == 1)) fail(DFDB_ERR_BOUNDS, "BoundsError: indexing a scalar selection");
      return;
    }
    if (ns.kind == ST_INTEGER) { r.kind = ST_INTEGER; r.idx = {last->elem(ns.idx[0])}; }
    else if (last->kind == ST_RANGE && ns.kind == ST_RANGE) {
      r.kind = ST_RANGE; r.step = last->step * ns.step;
      if (ns.n == 0) { r.start = last->start; r.stop = r.start - r.step; }
      else { r.start = last->elem(ns.start); r.stop = last->elem(ns.stop); }
    } else {
      r.kind = ST_INDICES; r.idx.resize((size_t)ns.n);
      for (int64_t k = 0; k < ns.n; k++) r.idx[(size_t)k] = last->elem(ns.kind == ST_RANGE ? ns.start + k * ns.step : ns.idx[(size_t)k]);
    }
    normalise(r);
    *last = std::move(r);
    return;
  }
  if (last && last->kind == ST_PRED && !new_is_range) {   // predicate∘predicate fuses with & (:44-47)
    last->pred = make_and(std::move(last->pred), std::move(ns.pred));
    return;
  }
  q->stages.push_back(std::move(ns));
}

// ---------------------------------------------------------------- device state
size_t padded_words(int64_t nrows) { return (size_t)(round_up(nrows > 0 ? nrows : 1, kCTileRows) / 64 + 64); }

static void ensure_state(dfdb_query* q) {
  dfdb_table* t = q->t;
  if (t->nrows < 0) fail(DFDB_ERR_ARGUMENT, "table has no resident columns: call dfdb_table_load / add_column first");
  const int64_t nrows = t->nrows;
  if (q->bitmap_rows != nrows) {
    const size_t nw = padded_words(nrows);
    const int64_t ntiles = ceil_div(nrows, kTileRows);
    q->bitmap.ensure(nw * 8);
    HIP_CHECK(hipMemsetAsync(q->bitmap.p, 0, nw * 8, t->ctx->stream));   // pad words stay zero forever
    q->tile_counts.ensure((size_t)(ntiles + 8) * 4);
    q->prefix.ensure((size_t)(ntiles + 8) * 8);
    HIP_CHECK(hipMemsetAsync(q->prefix.p, 0, (size_t)(ntiles + 8) * 8, t->ctx->stream));
    q->scan_scratch.ensure(scan_counts_scratch_bytes(ntiles));
    q->bitmap_rows = nrows;
    q->executed_stages = -1;
  }
}

// ---------------------------------------------------------------- placement calibration
// K1 reads a column at ~7 TB/s while writing 1/64 of that as the bitmap.  How fast the pair runs depends on WHERE the two allocations sit
// relative to each other in physical memory (tools/bench_offset: every 8-GB column timed against every one of twelve bitmap allocations —
// 1.18 ms for some pairs, 1.32 ms for others, repeatably; offsets INSIDE an allocation change nothing), presumably DRAM bank conflicts between
// the read stream and the open bitmap rows under the address hash.  Neither hipMalloc nor the virtual-memory API lets the caller choose
// physical placement, so the engine measures: the first time a column of >= 2^26 rows is the target of a fresh-mask scan, the scan is timed
// against a few candidate bitmap allocations spread over free HBM (spacer allocations in between, released
// afterwards) and the fastest stays with the column.  Queries that scan the column borrow it (one at a time; others use their own).
// ctx option "placement_calibrate" = 1 asks for it (default 0).  One-time cost per column: 27 scans (~35 ms per 1e9 rows) plus allocating and releasing
// the spacers, 0.03-1.4 s measured (profiles/r2_placement_cost.txt) — worth it for a column that stays resident and is scanned thousands of times, not
// for a short session, which is why it is opt-in; stream slots never calibrate.  "placement_spacer_mb" / "placement_candidates" size the search (round 3: no
// spacers by default — once the column itself is re-placed they change nothing, tools/r3_draws_spacer.sh, and releasing 8 x 12 GB of them was up to 5 s of the one-time cost).
void query_return_mask(dfdb_query* q) {
  if (q->mask_from < 0 || !q->t) { q->mask_from = -1; return; }
  Column& c = q->t->cols[(size_t)q->mask_from];
  std::swap(q->bitmap, c.mask_pref); c.mask_lent = false; q->mask_from = -1;
  q->executed_stages = -1; q->count = -1; q->prefix_valid = false;
}
// Round 3: it is the COLUMN's allocation that decides most of it.  Six 8-GB columns with the same contents in one process (tools/r3_column_placement.py): one
// scans at 1.19-1.20 ms whatever bitmap it is paired with, one at 1.25-1.30, four at 1.28-1.32 — the nine bitmap candidates of one column differ by 1-4 %, the
// columns by 9 %.  So the calibration first RE-PLACES the column: a few fresh allocations of its size (all held until the choice is made: a freed one would be
// handed out again), the data copied device to device, the scan timed on each against the query's own bitmap; the fastest allocation becomes the column.
// "placement_column_candidates" (default 8, at most 16; 0 = bitmaps only).  Costs candidates x (the column's size of free HBM + a copy + 3 scans), once per column.
template <class Launch>
static void place_mask(dfdb_query* q, int ordinal, Launch&& launch /* (uint64_t* bitmap, int64_t rows, const void* column) */) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const int64_t nrows = t->nrows;
  if (nrows < ((int64_t)1 << 26) || ctx_option(ctx, "placement_calibrate", 0) == 0) return;
  if (q->mask_from == ordinal) return;
  query_return_mask(q);
  Column& c = t->cols[(size_t)ordinal];
  const size_t bytes = padded_words(nrows) * 8;
  if (!c.mask_calibrated) {
    c.mask_calibrated = true;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return; }
    const auto wall0 = std::chrono::steady_clock::now();
    const int kCand = 8;                    // candidate bitmaps (round 6: the A/B knobs of the search — "placement_candidates", "placement_spacer_mb", "placement_count_candidates" — are constants now)
    const size_t spacer = 0;              // (round 2 held 12 GB between the candidates: seconds to release, nothing gained once the column is re-placed)
    if (free_b < (size_t)kCand * (bytes + spacer) + ((size_t)4 << 30)) return;      // not enough room to look around: keep the query's own
    std::vector<DevBuf> cand((size_t)kCand), space((size_t)kCand);
    try {
      for (int k = 0; k < kCand; k++) { cand[(size_t)k].ensure(bytes); if (spacer >= ((size_t)64 << 20)) space[(size_t)k].ensure(spacer); }
    } catch (const Error&) { return; }
    const int64_t sample = nrows;      // the WHOLE column: how a bitmap allocation pairs with the first eighth says little about the rest (measured)
    struct EventPair {                 // (a HIP_CHECK that throws inside time_on must not leak them: ADVICE r3)
      hipEvent_t a = nullptr, b = nullptr;
      ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b));
    const hipEvent_t e0 = ev.a, e1 = ev.b;
    const void* colp = c.data.p;
    auto time_on = [&](uint64_t* bm) {
      float best = 1e30f;
      for (int r = 0; r < 3; r++) {
        HIP_CHECK(hipEventRecord(e0, s));
        launch(bm, sample, colp);
        HIP_CHECK(hipEventRecord(e1, s));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r > 0 && ms < best) best = ms;
      }
      return best;
    };
    // ---- the column first
    const int kCol = (int)std::min<int64_t>(16, std::max<int64_t>(0, ctx_option(ctx, "placement_column_candidates", 8)));
    if (kCol > 0 && dt_base(c.dtype) != DFDB_STRING && c.data.bytes > 0 && free_b > (size_t)(kCol + 1) * c.data.bytes + (size_t)kCand * (bytes + spacer) + ((size_t)8 << 30)) {
      std::vector<DevBuf> ccand((size_t)kCol);
      float tcol = time_on(q->bitmap.as<uint64_t>()), tcol_worst = tcol; int cbest = -1;
      for (int k = 0; k < kCol; k++) {
        try { ccand[(size_t)k].ensure(c.data.bytes); } catch (const Error&) { break; }
        HIP_CHECK(hipMemcpyAsync(ccand[(size_t)k].p, c.data.p, c.data.bytes, hipMemcpyDeviceToDevice, s));
        colp = ccand[(size_t)k].p;
        const float tk = time_on(q->bitmap.as<uint64_t>());
        if (tk < tcol) { tcol = tk; cbest = k; }
        if (tk > tcol_worst) tcol_worst = tk;
      }
      auto& pcb = ctx->prof["placement_column_best_us"]; pcb.launches++; pcb.ms += tcol * 1e3;
      auto& pcw = ctx->prof["placement_column_worst_us"]; pcw.launches++; pcw.ms += tcol_worst * 1e3;
      HIP_CHECK(hipStreamSynchronize(s));
      if (cbest >= 0 && tcol < 0.985f * tcol_worst) std::swap(c.data, ccand[(size_t)cbest]);      // the column lives in the fastest allocation from now on
      colp = c.data.p;
      ccand.clear();                                      // the others (and the old one) go back
    }
    float tbest = time_on(q->bitmap.as<uint64_t>()), tworst = tbest; int kbest = -1;
    for (int k = 0; k < kCand; k++) {
      const float tk = time_on(cand[(size_t)k].as<uint64_t>());
      if (tk < tbest) { tbest = tk; kbest = k; }
      if (tk > tworst) tworst = tk;
    }
    // ---- the query's tile-count array last (4 bytes per 1024 rows: K1 writes it beside the bitmap).  Its placement is worth 1-2.5 % of the scan (eight candidates in each
    // of six processes: 1.195-1.236 ms), the search costs a few 4-MB allocations and 3 scans each: "placement_count_candidates" (default 4, 0 = leave it)
    const int kTc = 4;
    if (kTc > 0 && q->tile_counts.bytes > 0) {
      uint64_t* const bmx = kbest >= 0 ? cand[(size_t)kbest].as<uint64_t>() : q->bitmap.as<uint64_t>();
      std::vector<DevBuf> tcand((size_t)kTc);
      float tc_best = time_on(bmx), tc_worst = tc_best; int tc_k = -1;
      for (int k = 0; k < kTc; k++) {
        try { tcand[(size_t)k].ensure(q->tile_counts.bytes); } catch (const Error&) { break; }
        std::swap(q->tile_counts, tcand[(size_t)k]);
        const float tk = time_on(bmx);
        std::swap(q->tile_counts, tcand[(size_t)k]);
        if (tk < tc_best) { tc_best = tk; tc_k = k; }
        if (tk > tc_worst) tc_worst = tk;
      }
      auto& pcb = ctx->prof["placement_counts_best_us"]; pcb.launches++; pcb.ms += tc_best * 1e3;
      auto& pcw = ctx->prof["placement_counts_worst_us"]; pcw.launches++; pcw.ms += tc_worst * 1e3;
      HIP_CHECK(hipStreamSynchronize(s));
      if (tc_k >= 0) std::swap(q->tile_counts, tcand[(size_t)tc_k]);
    }
    c.mask_ms_best = tbest; c.mask_ms_worst = tworst;
    auto& pe = ctx->prof["placement_best_us"]; pe.launches++; pe.ms += tbest * 1e3;
    auto& pw = ctx->prof["placement_worst_us"]; pw.launches++; pw.ms += tworst * 1e3;
    if (kbest >= 0 && tbest < 0.985f * tworst) {       // a real difference, and the query's own allocation is not the winner
      c.mask_pref = std::move(cand[(size_t)kbest]);
      HIP_CHECK(hipMemsetAsync(c.mask_pref.p, 0, bytes, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));                 // candidates and spacers die here
    HIP_CHECK(hipMemsetAsync(q->bitmap.p, 0, bytes, s));
    cand.clear(); space.clear();                        // (freed inside the timed span: releasing the spacers is most of the cost)
    auto& pt = ctx->prof["placement_wall_us"]; pt.launches++;
    pt.ms += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - wall0).count();
  }
  if (c.mask_pref.p && !c.mask_lent && c.mask_pref.bytes >= bytes) {
    std::swap(q->bitmap, c.mask_pref); c.mask_lent = true; q->mask_from = ordinal;
  }
}

uint64_t splitmix64_host(uint64_t x) { x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); }

// (a compressed-only column — keep_compressed = 2 — that reaches a consumer through here gets a whole-column decode for the ABI call in progress:
//  table.cpp column_data; the paths that need none — K7's fused scan, the survivors' arena of the gathers — do not come through here)
const Column& need_resident(dfdb_table* t, int ordinal) {
  Column& c = t->cols[(size_t)ordinal];
  if (!c.resident) fail(DFDB_ERR_ARGUMENT, "column %s is not resident on the device (dfdb_table_load it first)", c.name.c_str());
  if (c.comp_only) (void)column_data(t, c);
  return c;
}
// can K7 itself evaluate this simple term over a compressed-only column (HIST + SCAN: decode and compare in one pass, nothing decoded is kept)?
static bool comp_scannable(const dfdb_table* t, const ScanTerm& tm, int ord) {
  const Column& c = t->cols[(size_t)ord];
  return c.resident && c.comp_only && !c.data.p && tm.pre == 0 && (tm.dtype == DFDB_I64 || tm.dtype == DFDB_U64 || tm.dtype == DFDB_F64) && !dt_nullable(c.dtype) &&
         t->block_size % kTileRows == 0;
}

static void raise_reached_errors(dfdb_query* q, int nstages);
// The bitmap was changed outside query_execute (unique narrowed it to the first occurrences, groupreduce put the full selection back): everything derived
// from the PREVIOUS bitmap goes — the host count, and the survivors' arenas of compressed-only projection columns, which hold only the blocks that kept a
// row under the selection they were decoded for (a fetch restored the full selection and a later materialize gathered through the narrowed arena).
void selection_changed(dfdb_query* q) {
  q->count = -1;
  for (auto& a : q->arenas) a.second.valid = false;
}
void scan_prefix(dfdb_query* q) {
  dfdb_ctx* ctx = q->t->ctx;
  LaunchTimer lt(ctx, "scan_counts");
  launch_scan_counts(ctx->stream, q->tile_counts.as<uint32_t>(), q->prefix.as<uint64_t>(), ceil_div(q->t->nrows, kTileRows), q->scan_scratch.as<uint64_t>());
  q->prefix_valid = true;
}

// K9: does dictionary entry `e` satisfy the string term (mode 0 ==, 1 !=, 2 startswith, 3 endswith; k_strings.hip's modes)?
static bool dict_entry_matches(const std::string& e, int mode, const std::string& pat) {
  if (mode <= 1) { const bool r = e == pat; return mode == 1 ? !r : r; }
  if (mode == 2) return e.size() >= pat.size() && e.compare(0, pat.size(), pat) == 0;
  return e.size() >= pat.size() && e.compare(e.size() - pat.size(), pat.size(), pat) == 0;
}
static void run_dict_scan(dfdb_query* q, const Column& col, const std::vector<uint32_t>& lut, bool have) {
  dfdb_ctx* ctx = q->t->ctx; hipStream_t s = ctx->stream;
  DevBuf& lb = q->tmp_a; lb.ensure(lut.size() * 4 + 64);
  HIP_CHECK(hipMemcpyAsync(lb.p, lut.data(), lut.size() * 4, hipMemcpyHostToDevice, s));
  stream_wait(ctx);                                      // `lut` is pageable host memory
  LaunchTimer lt(ctx, "dict_scan");
  launch_dict_scan(s, col.dict_codes.as<uint16_t>(), lb.as<uint32_t>(), (int32_t)lut.size(), q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), q->t->nrows, have);
}
// s1 OP s2 over two dictionary columns: the two dictionaries merged on every run of the conjunct (not cached: at most 65535 entries each) — the union sorted bytewise (std::string orders as memcmp then length, bytes
// unsigned: Base.cmp), equal strings one rank — and one rank table per column uploaded; the rows compare ranks (k_dict_pair)
static void run_dict_pair(dfdb_query* q, const Column& ca, const Column& cb, int op, bool have) {
  dfdb_ctx* ctx = q->t->ctx; hipStream_t s = ctx->stream;
  const size_t na = (size_t)ca.dict_n, nb = (size_t)cb.dict_n;
  std::vector<const std::string*> all; all.reserve(na + nb);
  for (const std::string& e : ca.dict_host) all.push_back(&e);
  for (const std::string& e : cb.dict_host) all.push_back(&e);
  std::vector<uint32_t> order(na + nb), rank(na + nb);
  for (size_t k = 0; k < order.size(); k++) order[k] = (uint32_t)k;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return *all[x] < *all[y]; });
  uint32_t r = 0;
  for (size_t k = 0; k < order.size(); k++) { if (k && *all[order[k]] != *all[order[k - 1]]) r++; rank[order[k]] = r; }
  DevBuf& rb = q->tmp_a; rb.ensure(rank.size() * 4 + 64);
  HIP_CHECK(hipMemcpyAsync(rb.p, rank.data(), rank.size() * 4, hipMemcpyHostToDevice, s));
  stream_wait(ctx);                                      // `rank` is pageable host memory
  LaunchTimer lt(ctx, "dict_pair");
  launch_dict_pair(s, ca.dict_codes.as<uint16_t>(), cb.dict_codes.as<uint16_t>(), rb.as<uint32_t>(), (int32_t)na, rb.as<uint32_t>() + na, (int32_t)nb, op,
                   q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), q->t->nrows, have);
}

// predicate stage = AND of its conjuncts, each routed to the cheapest kernel that is exact for it
static void run_predicate(dfdb_query* q, const Node& pred, bool first_stage, bool last_stage) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const int64_t nrows = t->nrows;
  std::vector<const Node*> conj; flatten_and(pred, conj);
  std::vector<const Node*> generic, strs; ScanTerms terms{}; terms.n = 0; terms.combine_or = 0;
  std::vector<ScanTerms> term_batches;
  std::vector<int> term_ords;
  // a conjunct that is itself a disjunction of simple terms — (a > c1) | (x < c2) — is one k_scan_terms pass with combine_or
  std::vector<ScanTerms> or_batches;
  auto match_or = [&](const Node& n, ScanTerms& out) {
    std::vector<const Node*> leaves, todo{&n};
    while (!todo.empty()) {
      const Node* x = todo.back(); todo.pop_back();
      if (x->op == DFIR_OR && x->a && x->b) { todo.push_back(x->b.get()); todo.push_back(x->a.get()); } else leaves.push_back(x);
    }
    out = ScanTerms{}; out.n = 0; out.combine_or = 1;
    for (const Node* l : leaves) {
      // in.(col, Ref([v1, v2, ...])) (test/broadcast.jl:63-71) with a few values is the disjunction col == v1 | col == v2 | ...
      if (l->op == DFIR_IN_SET && l->a && l->b && l->a->op == DFIR_COL && l->b->op == DFIR_CONST_SET && !l->b->set.empty()) {
        for (uint64_t bits : l->b->set) {
          Node eq; eq.op = DFIR_EQ; eq.dtype = DFDB_BOOL;
          eq.a = l->a->clone();
          eq.b = std::make_unique<Node>(); eq.b->op = DFIR_CONST; eq.b->dtype = l->b->set_dtype; eq.b->cbits = bits;
          ScanTerm tm; int ord;
          if (out.n == kMaxTerms || !match_simple_term(eq, *t, tm, ord)) return false;
          tm.col = need_resident(t, ord).data.p;
          out.t[out.n++] = tm;
        }
        continue;
      }
      ScanTerm tm; int ord;
      if (out.n == kMaxTerms || !match_simple_term(*l, *t, tm, ord)) return false;
      tm.col = need_resident(t, ord).data.p;
      out.t[out.n++] = tm;
    }
    return out.n >= 2;
  };
  // ismissing(col) / !ismissing(col) over a nullable fixed-width column: its missing bitmap is the mask
  // a disjunction (and negations) of string terms over ONE dictionary column — (brand == "sony") | (brand == "apple"), !startswith(brand, "x") — is a
  // Boolean function of the dictionary entry: one bit-table lookup of the codes instead of string compares in the interpreter
  struct DictLut { int ord; std::vector<uint32_t> lut; };
  std::vector<DictLut> dict_luts;
  std::function<bool(const Node&, int&)> dict_only = [&](const Node& n, int& ord) -> bool {
    if ((n.op == DFIR_OR || n.op == DFIR_AND || n.op == DFIR_XOR) && n.a && n.b) return dict_only(*n.a, ord) && dict_only(*n.b, ord);
    if (n.op == DFIR_NOT && n.a) return dict_only(*n.a, ord);
    int o, mode; std::string pat;
    if (!match_string_term(n, *t, o, mode, pat)) return false;
    if (ord >= 0 && o != ord) return false;
    if (t->cols[(size_t)o].dict_n <= 0 || !t->cols[(size_t)o].resident) return false;
    ord = o; return true;
  };
  std::function<bool(const Node&, const std::string&)> dict_eval = [&](const Node& n, const std::string& e) -> bool {
    if (n.op == DFIR_OR) return dict_eval(*n.a, e) || dict_eval(*n.b, e);
    if (n.op == DFIR_AND) return dict_eval(*n.a, e) && dict_eval(*n.b, e);
    if (n.op == DFIR_XOR) return dict_eval(*n.a, e) != dict_eval(*n.b, e);
    if (n.op == DFIR_NOT) return !dict_eval(*n.a, e);
    int o, mode; std::string pat; match_string_term(n, *t, o, mode, pat);
    return dict_entry_matches(e, mode, pat);
  };
  // `s1 OP s2` over two String columns (and coalesce(s1 OP s2, false) over nullable ones): k_str_pair / k_dict_pair; ctx option "str_pair_kernel" = 0 leaves
  // it to the interpreter's H_STRCMP2, which is the definition
  struct PairTerm { int a, b, op; };
  std::vector<PairTerm> pairs;
  const bool pair_kernel = ctx_option(ctx, "str_pair_kernel", 1) != 0;
  struct MissTerm { const uint64_t* bits; bool negate; };
  std::vector<MissTerm> miss;
  struct CompTerm { ScanTerm tm; int ord; };
  std::vector<CompTerm> comp_terms;
  auto match_missing = [&](const Node& n, MissTerm& out) {
    const Node* m = &n; bool neg = false;
    if (m->op == DFIR_NOT && m->a) { m = m->a.get(); neg = true; }
    if (m->op != DFIR_ISMISSING || !m->a || m->a->op != DFIR_COL) return false;
    const Column& col = need_resident(t, m->a->col);
    if (!dt_nullable(col.dtype) || dt_base(col.dtype) == DFDB_STRING || !col.missing.p) return false;
    out = MissTerm{col.missing.as<uint64_t>(), neg};
    return true;
  };
  for (const Node* c : conj) {
    ScanTerm tm; int ord; int mode; std::string pat;
    ScanTerms ob;
    MissTerm mt;
    if (match_missing(*c, mt)) { miss.push_back(mt); continue; }
    if (c->op == DFIR_OR || c->op == DFIR_NOT || c->op == DFIR_XOR) {
      int dord = -1;
      if (dict_only(*c, dord) && dord >= 0) {
        const Column& dc = t->cols[(size_t)dord];
        DictLut dl{dord, std::vector<uint32_t>((size_t)(dc.dict_n + 31) / 32, 0u)};
        for (int32_t k = 0; k < dc.dict_n; k++) if (dict_eval(*c, dc.dict_host[(size_t)k])) dl.lut[(size_t)k >> 5] |= 1u << (k & 31);
        dict_luts.push_back(std::move(dl));
        continue;
      }
    }
    if ((c->op == DFIR_OR || c->op == DFIR_IN_SET) && match_or(*c, ob)) { or_batches.push_back(ob); continue; }
    const bool simple = match_simple_term(*c, *t, tm, ord);      // (once: a failed match leaves `tm` half-written)
    if (simple && comp_scannable(t, tm, ord)) {
      // a compressed-only column: the decoder evaluates the term (a second comparison of the same column folds into an interval there too)
      bool folded = false;
      for (CompTerm& ct : comp_terms) if (ct.ord == ord && ct.tm.op2 < 0 && ct.tm.dtype == tm.dtype) { ct.tm.op2 = tm.op; ct.tm.cbits2 = tm.cbits; folded = true; break; }
      if (!folded) comp_terms.push_back(CompTerm{tm, ord});
      continue;
    }
    if (simple) {
      tm.col = need_resident(t, ord).data.p;
      // a second comparison of a column the current batch already compares folds into that term as an interval: `65 > x > 34`
      // (test/selection.jl:53) reads x once instead of twice
      bool folded = false;
      const size_t ord0 = term_ords.size() - (size_t)terms.n;
      for (int k = 0; k < terms.n && !folded; k++)
        if (term_ords[ord0 + (size_t)k] == ord && terms.t[k].op2 < 0 && terms.t[k].dtype == tm.dtype && terms.t[k].pre == tm.pre &&
            (tm.pre == 0 || (terms.t[k].pre_d == tm.pre_d && terms.t[k].pre_magic == tm.pre_magic))) { terms.t[k].op2 = tm.op; terms.t[k].cbits2 = tm.cbits; folded = true; }
      if (folded) continue;
      if (terms.n == kMaxTerms) { term_batches.push_back(terms); terms.n = 0; }
      terms.t[terms.n++] = tm; term_ords.push_back(ord);
    } else if (match_string_term(*c, *t, ord, mode, pat)) strs.push_back(c);
    else if (c->op == DFIR_COALESCE && c->a && c->b && c->b->op == DFIR_CONST && dt_base(c->b->dtype) == DFDB_BOOL && !dt_nullable(c->b->dtype) && c->b->cbits == 0 &&
             match_string_term(*c->a, *t, ord, mode, pat, true))
      strs.push_back(c->a.get());     // coalesce(s == "x", false) over a Union{String,Missing} column (the docs' real data set: index.md:264-272): K5's own answer, not the interpreter's
    else if (PairTerm pt{}; pair_kernel && match_string_pair_term(*c, pt.a, pt.b, pt.op)) pairs.push_back(pt);
    else if (PairTerm pt{}; pair_kernel && c->op == DFIR_COALESCE && c->a && c->b && c->b->op == DFIR_CONST && dt_base(c->b->dtype) == DFDB_BOOL && !dt_nullable(c->b->dtype) &&
             c->b->cbits == 0 && match_string_pair_term(*c->a, pt.a, pt.b, pt.op, true))
      pairs.push_back(pt);
    else generic.push_back(c);
  }
  if (terms.n) term_batches.push_back(terms);
  bool have = !first_stage;   // does the bitmap already hold a mask to AND with?
  // generic conjuncts first, as ONE interpreter program over `c1 & c2 & ...`: Julia's fused `&` is not short-circuit
  // (BlockBroadcasting(&, (old, elem)), selection.jl:44-47), so every conjunct is evaluated — and may raise DivideError /
  // InexactError — on every row that REACHED this stage, not only on the rows an earlier conjunct kept
  if (generic.size() == 1) { run_interp_predicate(q, *generic[0], have); have = true; }
  else if (!generic.empty()) {
    NodePtr all = generic[0]->clone();
    for (size_t i = 1; i < generic.size(); i++) all = make_and(std::move(all), generic[i]->clone());
    run_interp_predicate(q, *all, have); have = true;
  }
  for (const DictLut& dl : dict_luts) { run_dict_scan(q, t->cols[(size_t)dl.ord], dl.lut, have); have = true; }
  for (const Node* c : strs) {
    int ord, mode; std::string pat; match_string_term(*c, *t, ord, mode, pat, true);
    const Column& col = need_resident(t, ord);
    const bool str_nullable = dt_nullable(col.dtype);
    // `col == "const"` is an AND-ed conjunct of this stage, and later stages only remove rows: every row the query finally selects holds exactly
    // `const` in this column, so its projection needs neither the column nor a capture (materialize_col: launch_fill_const_strings)
    if (mode == 0 && !str_nullable) { q->const_str_col = ord; q->const_str = pat; }
    if (col.dict_n > 0) {
      // K9: the column has a dictionary — the term is decided once per distinct string on the host, the rows are a bit-table lookup of their codes
      std::vector<uint32_t> lut((size_t)(col.dict_n + 31) / 32, 0u);
      for (int32_t k = 0; k < col.dict_n; k++) if (dict_entry_matches(col.dict_host[(size_t)k], mode, pat)) lut[(size_t)k >> 5] |= 1u << (k & 31);
      run_dict_scan(q, col, lut, have);
      have = true;
      continue;
    }
    DevBuf& pb = q->tmp_a; pb.ensure(pat.size() + 64);
    if (pat.size() > 16) { HIP_CHECK(hipMemcpyAsync(pb.p, pat.data(), pat.size(), hipMemcpyHostToDevice, s)); stream_wait(q->t->ctx); }   // (bytes past 16 are compared against the device copy)
    // capture (see dfdb_query.hint_materialize): only when this ONE launch produces the query's final mask and the column it reads is
    // itself projected — the match pass then keeps the selected rows' sizes and bytes and K6 never reads the column again
    StrCapture capture{nullptr, nullptr, nullptr};
    // (every other kind of conjunct runs AFTER this launch and narrows the mask: the capture would keep rows the query drops — found by tests/test_gpu_fuzz.py)
    bool do_cap = mode != 0 && !str_nullable && q->hint_materialize && q->stages.size() == 1 && !have && generic.empty() && term_batches.empty() && or_batches.empty() && miss.empty() && comp_terms.empty() &&
                  dict_luts.empty() && strs.size() == 1 && pairs.empty() && pat.size() <= 64;
    if (do_cap) {
      do_cap = false;
      for (const ProjCol& p : q->proj) if (p.expr->op == DFIR_COL && p.expr->col == ord) { do_cap = true; break; }
    }
    if (do_cap) {
      const int64_t nt = ceil_div(nrows, kTileRows);
      q->cap_str_sizes.ensure((size_t)nt * kTileRows * 4 + 256);
      q->cap_str_bytes.ensure((size_t)col.nbytes + 256);
      q->cap_str_tb.ensure((size_t)(nt + 8) * 4);
      capture = StrCapture{q->cap_str_sizes.as<int32_t>(), q->cap_str_bytes.as<uint8_t>(), q->cap_str_tb.as<uint32_t>()};
    }
    LaunchTimer lt(ctx, "str_match");
    launch_str_match(s, col.data.as<int32_t>(), (const int64_t*)col.tile_off.p, col.bytes.as<uint8_t>(), (const uint8_t*)pat.data(),
                     pb.as<uint8_t>(), (int32_t)pat.size(), mode, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), nrows, have,
                     do_cap ? &capture : nullptr, col.max_tile_bytes);
    if (do_cap) q->cap_str_col = ord;
    have = true;
  }
  // (after the generic conjuncts like every other string scan: those see every row that reached the stage; a pair launch pins no constant and captures nothing)
  for (const PairTerm& pt : pairs) {
    const Column& ca = need_resident(t, pt.a);
    const Column& cb = need_resident(t, pt.b);
    if (ca.dict_n > 0 && cb.dict_n > 0) { run_dict_pair(q, ca, cb, pt.op, have); have = true; continue; }      // (a dictionary column is never nullable)
    LaunchTimer lt(ctx, "str_pair");
    launch_str_pair(s, ca.data.as<int32_t>(), (const int64_t*)ca.tile_off.p, ca.bytes.as<uint8_t>(), cb.data.as<int32_t>(), (const int64_t*)cb.tile_off.p,
                    cb.bytes.as<uint8_t>(), pt.op, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), nrows, have);
    have = true;
  }
  for (const MissTerm& mt : miss) {
    LaunchTimer lt(ctx, "missing_mask");
    launch_missing_mask(s, mt.bits, mt.negate, have, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), nrows);
    have = true;
  }
  for (const ScanTerms& ob : or_batches) {
    LaunchTimer lt(ctx, "scan_terms");
    launch_scan_terms(s, ob, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), nrows, have, 0, nullptr);
    have = true;
  }
  // compressed-only columns: one K7 launch per term — every block decoded into the waves' history rings, the comparison applied to the bytes as they leave
  // the LDS ring, bitmap + tile counts the only output.  From the second mask on the words are AND-ed in and a block without a survivor
  // is not decoded at all (blocksiterator.jl:111-113 at block granularity).
  for (const CompTerm& ct : comp_terms) {
    Column& fc = t->cols[(size_t)ct.ord];
    LzScan sc{q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), ct.tm.cbits, ct.tm.dtype, ct.tm.op};
    sc.op2 = ct.tm.op2; sc.cbits2 = ct.tm.cbits2; sc.and_existing = have ? 1 : 0;
    int waves = 0; uint8_t* scratch = ctx_hist_scratch(ctx, &waves);
    const int imode = column_lz4_index(ctx, fc, true);
    LaunchTimer lt(ctx, "lz4_decode_scan_hist");
    prof_note(ctx, imode == 2 ? "lz4_decode_scan_hist.indexed" : imode == 1 ? "lz4_decode_scan_hist.recording" : "lz4_decode_scan_hist.plain");
    launch_lz4_decode_hist(s, fc.comp.as<uint8_t>(), scratch, waves, fc.comp_blocks.as<Lz4Block>(), (int32_t)fc.comp_nblocks, fc.comp_status.as<int32_t>(), &sc,
                           fc.comp_index.as<uint32_t>(), imode);
    if (std::find(q->comp_scanned.begin(), q->comp_scanned.end(), ct.ord) == q->comp_scanned.end()) q->comp_scanned.push_back(ct.ord);
    have = true;
  }
  // The launch that produces the query's final mask can do more with its LAST term (k_scan_terms EXTRA):
  //   sum     (dfdb_query_hint_aggregate): the hinted column is a term of the last batch of the last stage -> per-tile partial sums
  //   capture (dfdb_query_hint_materialize): a single-stage query of one batch of terms, one of them a projected 8-byte column
  int extra = 0, special = -1;
  if (!term_batches.empty() && !term_batches.back().combine_or) {
    ScanTerms& lb = term_batches.back();
    const size_t ord0 = term_ords.size() - (size_t)lb.n;           // term_ords of the last batch start here
    if ((q->hint_agg_op == DFDB_AGG_SUM || q->hint_agg_op == DFDB_AGG_MIN || q->hint_agg_op == DFDB_AGG_MAX) && last_stage && q->hint_agg_proj >= 0 &&
        (size_t)q->hint_agg_proj < q->proj.size()) {
      const Node& pe = *q->proj[(size_t)q->hint_agg_proj].expr;
      if (pe.op == DFIR_COL && !dt_nullable(pe.dtype))
        for (int k = 0; k < lb.n && special < 0; k++) {
          const int dt = lb.t[k].dtype;
          if (lb.t[k].pre) continue;                              // (a rem term compares rem(x, m): not the value to add up)
          if (term_ords[ord0 + (size_t)k] == pe.col && (dt == DFDB_I64 || dt == DFDB_U64 || dt == DFDB_F64)) {
            special = k; extra = q->hint_agg_op == DFDB_AGG_SUM ? 2 : (q->hint_agg_op == DFDB_AGG_MIN ? 3 : 4);
          }
        }
    }
    // capture: the last batch of the LAST stage is the launch that produces the query's final mask, whatever ran before it in this stage (generic
    // conjuncts, string and dictionary scans, missing masks, disjunctions all come first and only hand it a mask to AND with) or in earlier stages.
    // Every projected plain 8-byte column among its terms — up to two — is kept by the scan instead of gathered afterwards (round 4; round 1-3 captured
    // one column of a single-stage query whose only conjuncts were simple terms).
    int special2 = -1;
    if (!extra && q->hint_materialize && last_stage && ctx_option(ctx, "scan_capture", 2) > 0) {
      const int maxcap = (int)std::min<int64_t>(2, ctx_option(ctx, "scan_capture", 2));
      for (int k = 0; k < lb.n && (special < 0 || (special2 < 0 && maxcap >= 2)); k++) {
        const int dt = lb.t[k].dtype;
        if ((dt != DFDB_I64 && dt != DFDB_U64 && dt != DFDB_F64) || lb.t[k].pre) continue;
        if (special >= 0 && term_ords[ord0 + (size_t)k] == term_ords[ord0 + (size_t)special]) continue;     // (two terms of one column that did not fold)
        for (const ProjCol& p : q->proj) {
          bool wanted = p.expr->op == DFIR_COL && p.expr->col == term_ords[ord0 + (size_t)k] && !dt_nullable(p.expr->dtype);
          if (!wanted && p.expr->op != DFIR_COL && dt_width(p.expr->dtype) == 8 && !dt_nullable(p.expr->dtype)) {
            // a computed column that is a transform of this one column (`x * 2`, `a % 7`, `a * 3 + 1`): it is made from the captured values too
            ScanTerm tf; const Node* tcol = nullptr;
            wanted = match_column_transform(p.expr.get(), tf, tcol) && tf.pre != 0 && tcol->col == term_ords[ord0 + (size_t)k] && !dt_nullable(tcol->dtype);
          }
          if (wanted) { if (special < 0) { special = k; extra = 1; } else { special2 = k; extra = 5; } break; }
        }
      }
    }
    if (extra) {                                                     // the special term goes last (and the second captured one before it)
      std::swap(lb.t[special], lb.t[lb.n - 1]);
      std::swap(term_ords[ord0 + (size_t)special], term_ords[ord0 + (size_t)lb.n - 1]);
      if (extra == 5) {
        if (special2 == lb.n - 1) special2 = special;                // (it was sitting in the last place and has just been swapped away)
        std::swap(lb.t[special2], lb.t[lb.n - 2]);
        std::swap(term_ords[ord0 + (size_t)special2], term_ords[ord0 + (size_t)lb.n - 2]);
        q->cap_buf2.ensure((size_t)round_up(nrows, kTileRows) * 8 + 256);
      }
      if (extra == 1 || extra == 5) q->cap_buf.ensure((size_t)round_up(nrows, kTileRows) * 8 + 256);
      else q->agg_partials.ensure((size_t)(ceil_div(nrows, kTileRows) + 8) * 8);
    }
  }
  if (!have && !term_batches.empty() && first_stage) {
    // the launch that writes a fresh mask over the whole column: run it against the bitmap allocation this column pairs best with
    const ScanTerms tb0 = term_batches[0];
    const bool nt = true;                 // nontemporal column loads (the A/B knob "scan_nt" went in round 6: plain loads were never faster)
    const int wt0 = (ctx_option(ctx, "scan_wt_store", 1) ? 1 : 0) | (int)((ctx_option(ctx, "scan_narrow", 1) & 3) << 1);
    const void* const col_before = t->cols[(size_t)term_ords[0]].data.p;
    place_mask(q, term_ords[0], [&](uint64_t* bm, int64_t rows, const void* colp) {
      ScanTerms tbx = tb0;                                          // the calibration may be trying another allocation of the first term's column
      for (int k = 0; k < tbx.n; k++) if (tbx.t[k].col == col_before) tbx.t[k].col = colp;
      if (tbx.n == 1 && tbx.t[0].op2 < 0 && tbx.t[0].pre == 0) launch_scan_cmp(s, tbx.t[0].col, tbx.t[0].dtype, tbx.t[0].op, tbx.t[0].cbits, bm, q->tile_counts.as<uint32_t>(), rows, false, nt, nullptr, wt0);
      else launch_scan_terms(s, tbx, bm, q->tile_counts.as<uint32_t>(), rows, false, 0, nullptr, (int)ctx_option(ctx, "scan_pair", 1));
    });
    const void* const col_after = t->cols[(size_t)term_ords[0]].data.p;
    if (col_after != col_before) {                                  // the column was re-placed: every term of this stage that reads it follows
      for (ScanTerms& tbk : term_batches) for (int k = 0; k < tbk.n; k++) if (tbk.t[k].col == col_before) tbk.t[k].col = col_after;
      for (ScanTerms& tbk : or_batches) for (int k = 0; k < tbk.n; k++) if (tbk.t[k].col == col_before) tbk.t[k].col = col_after;
    }
  }
  for (size_t bi = 0; bi < term_batches.size(); bi++) {
    const ScanTerms& tb = term_batches[bi];
    const int ex = bi + 1 == term_batches.size() ? extra : 0;
    // decode -> scan fusion: a fresh-mask scan of ONE simple term over an 8-byte column that holds its LZ4 blocks in HBM
    // (ctx option keep_compressed at load time) decodes the blocks and evaluates the term in the same pass (K7 SCAN): what the reference's loop
    // body does per block (read_block! then apply the selection, blocksiterator.jl:98-121).  ctx option "decode_on_scan" = 1 asks for it;
    // the decoded column is (re)written on the way, so everything after this launch sees an ordinary resident column.
    if (tb.n == 1 && tb.t[0].op2 < 0 && tb.t[0].pre == 0 && ex == 0 && !have && first_stage && bi == 0 && ctx_option(ctx, "decode_on_scan", 0) != 0) {
      Column& fc = t->cols[(size_t)term_ords[0]];
      const int fdt = tb.t[0].dtype;
      if (fc.comp_nblocks > 0 && !dt_nullable(fc.dtype) && (fdt == DFDB_I64 || fdt == DFDB_U64 || fdt == DFDB_F64) && t->block_size % kTileRows == 0) {
        q->decoded_col = term_ords[0];                   // query_count looks at the blocks' statuses where it waits for the count anyway
        // few blocks (every one resident in the two-wave pipeline at once): the pipeline, then the ordinary scan of the decoded column, is the shorter way —
        // a block's latency is what a small launch pays, and the fused form is one wave per block (1 526 blocks: 328 GB/s + a 0.13-ms scan against ~210 GB/s fused)
        const int pipe = (int)ctx_option(ctx, "lz4_pipeline", -1);
        if (pipe == 1 || (pipe < 0 && fc.comp_nblocks <= 2048)) {
          const int dmode = column_lz4_index(ctx, fc, lz4_decode_takes_index((int32_t)fc.comp_nblocks, pipe));
          LaunchTimer lt(ctx, "lz4_decode");
          prof_note(ctx, dmode == 2 ? "lz4_decode.indexed" : dmode == 1 ? "lz4_decode.recording" : "lz4_decode.plain");
          launch_lz4_decode(s, fc.comp.as<uint8_t>(), fc.data.as<uint8_t>(), fc.comp_blocks.as<Lz4Block>(), (int32_t)fc.comp_nblocks, fc.comp_status.as<int32_t>(), pipe,
                            fc.comp_index.as<uint32_t>(), dmode);
        } else {
        const int imode = column_lz4_index(ctx, fc, true);
        LaunchTimer lt(ctx, "lz4_decode_scan");
        prof_note(ctx, imode == 2 ? "lz4_decode_scan.indexed" : imode == 1 ? "lz4_decode_scan.recording" : "lz4_decode_scan.plain");
        launch_lz4_decode_scan(s, fc.comp.as<uint8_t>(), fc.data.as<uint8_t>(), fc.comp_blocks.as<Lz4Block>(), (int32_t)fc.comp_nblocks, fc.comp_status.as<int32_t>(),
                               LzScan{q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), tb.t[0].cbits, fdt, tb.t[0].op}, fc.comp_index.as<uint32_t>(), imode);
        have = true;
        continue;
        }
      }
    }
    if (tb.n == 1 && tb.t[0].op2 < 0 && tb.t[0].pre == 0 && ex < 2 && !(ex == 1 && have)) {      // (k_scan_cmp captures over a fresh mask only)
      LaunchTimer lt(ctx, "scan_cmp");
      prof_note(ctx, ctx_option(ctx, "scan_wt_store", 1) ? "scan_cmp.wt_store" : "scan_cmp.plain_store");
      launch_scan_cmp(s, tb.t[0].col, tb.t[0].dtype, tb.t[0].op, tb.t[0].cbits, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), nrows, have,
                      true, ex == 1 ? q->cap_buf.p : nullptr,
                      (ctx_option(ctx, "scan_wt_store", 1) ? 1 : 0) | (int)((ctx_option(ctx, "scan_narrow", 1) & 3) << 1));
    } else {
      LaunchTimer lt(ctx, "scan_terms");
      const int pair = (int)ctx_option(ctx, "scan_pair", 1);
      if (pair && scan_pair_applies(tb, have)) prof_note(ctx, "scan_terms.pair");
      launch_scan_terms(s, tb, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), nrows, have, ex, (ex == 1 || ex == 5) ? q->cap_buf.p : ex >= 2 ? q->agg_partials.p : nullptr, pair,
                        ex == 5 ? q->cap_buf2.p : nullptr);
    }
    have = true;
  }
  if (extra == 1 || extra == 5) q->cap_col = term_ords.back();
  if (extra == 5) q->cap_col2 = term_ords[term_ords.size() - 2];
  if (extra >= 2 && extra <= 4) { q->agg_col = term_ords.back(); q->agg_dtype = term_batches.back().t[term_batches.back().n - 1].dtype; q->agg_op = q->hint_agg_op; }
}

static void run_range(dfdb_query* q, const Stage& st, bool first_stage) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  RangeSpec r{};
  if (st.kind == ST_RANGE) {
    r.kind = 0; r.first = st.first(); r.last = st.last(); r.step = st.step > 0 ? st.step : -st.step;
    if (st.n == 0) { r.first = 1; r.last = 0; r.step = 1; }
  } else {   // index vectors keep table order and collapse duplicates (quirk Q3): membership in the sorted unique list
    std::vector<int64_t> sorted(st.idx);
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    q->idx_sorted.ensure(sorted.size() * 8 + 64);
    if (!sorted.empty()) HIP_CHECK(hipMemcpyAsync(q->idx_sorted.p, sorted.data(), sorted.size() * 8, hipMemcpyHostToDevice, s));
    stream_wait(q->t->ctx);   // `sorted` is pageable host memory
    r.kind = 1; r.sorted = q->idx_sorted.as<int64_t>(); r.nsorted = (int64_t)sorted.size();
    r.first = sorted.empty() ? 1 : sorted.front(); r.last = sorted.empty() ? 0 : sorted.back(); r.step = 1;
  }
  if (!first_stage && !q->prefix_valid) scan_prefix(q);
  // a leading range stage numbers TABLE rows (row_base makes that global on a shard); later stages number
  // the survivors, continuing after the survivors that live on lower ranks (stage_base)
  const int64_t rank_base = first_stage ? t->row_base : st.stage_base;
  LaunchTimer lt(ctx, "range_stage");
  launch_range_stage(s, r, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), q->tile_counts.as<uint32_t>(), t->nrows, rank_base, first_stage);
  q->prefix_valid = false;
}

// A predicate hit DivideError / InexactError on some rows.  Julia raises it only if the reference's iteration EVALUATES the block such a row lives in
// (src/io/blocksiterator.jl:69-121): blocks wholly before the first element of a leading range stage are skipped unread (skip_if_can,
// selection.jl:177-190), and once ANY range-like stage has been fed its last element (`last <= offset`, is_finished :192-196, tested before every block)
// nothing more is read.  `offset` of stage k before a block = the survivors of stages [0, k) in the rows before that block (+ stage_base on a shard).
// The rows before the erroring block raise nothing (it is the SMALLEST erroring row), so those counts come from ordinary partial executions.
static int64_t selected_before(dfdb_query* q, int64_t row) {                 // set bits of q's current bitmap in rows [0, row)
  dfdb_ctx* ctx = q->t->ctx; hipStream_t s = ctx->stream;
  const int64_t tile = row / kTileRows, words = (row % kTileRows) / 64, rem = row % 64;
  uint64_t pre = 0, w[17] = {0};
  HIP_CHECK(hipMemcpyAsync(&pre, q->prefix.as<uint64_t>() + tile, 8, hipMemcpyDeviceToHost, s));
  if (row % kTileRows) HIP_CHECK(hipMemcpyAsync(w, q->bitmap.as<uint64_t>() + tile * 16, (size_t)(words + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  int64_t c = (int64_t)pre;
  for (int64_t k = 0; k < words; k++) c += __builtin_popcountll(w[k]);
  if (rem) c += __builtin_popcountll(w[words] & ((1ull << rem) - 1ull));
  return c;
}
// survivors of the current execution in every block of `block_size` rows.  Blocks that are a whole number of 1024-row tiles read one entry of the
// prefix scan per block (a strided copy); other block sizes (the reference's tests use 50 and 100) count the bits of the mask on the host.
void query_block_counts(dfdb_query* q, int64_t block_size, std::vector<int64_t>& counts) {
  dfdb_table* t = q->t; hipStream_t s = t->ctx->stream;
  const int64_t nrows = t->nrows < 0 ? 0 : t->nrows;
  const int64_t nb = ceil_div(nrows, block_size);
  counts.assign((size_t)nb, 0);
  if (nb == 0) return;
  if (!q->prefix_valid) scan_prefix(q);
  const int64_t ntiles = ceil_div(nrows, kTileRows);
  if (block_size % kTileRows == 0) {
    const int64_t tpb = block_size / kTileRows;
    std::vector<uint64_t> at((size_t)nb + 1, 0);
    HIP_CHECK(hipMemcpy2DAsync(at.data(), 8, q->prefix.p, (size_t)tpb * 8, 8, (size_t)nb, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&at[(size_t)nb], q->prefix.as<uint64_t>() + ntiles, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (int64_t b = 0; b < nb; b++) counts[(size_t)b] = (int64_t)(at[(size_t)b + 1] - at[(size_t)b]);
    return;
  }
  const size_t nw = (size_t)ceil_div(nrows, 64);
  std::vector<uint64_t> bm(nw);
  HIP_CHECK(hipMemcpyAsync(bm.data(), q->bitmap.p, nw * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  for (int64_t b = 0; b < nb; b++) {
    const int64_t r0 = b * block_size, r1 = std::min(nrows, r0 + block_size);
    int64_t c = 0;
    for (int64_t r = r0; r < r1;) {
      const int64_t wi = r >> 6, lo = r & 63, hi = std::min<int64_t>(64, r1 - (wi << 6));
      uint64_t w = bm[(size_t)wi] >> lo;
      if (hi - lo < 64) w &= (1ull << (hi - lo)) - 1ull;
      c += __builtin_popcountll(w);
      r = (wi << 6) + hi;
    }
    counts[(size_t)b] = c;
  }
}

static bool error_is_reached(dfdb_query* q, uint64_t erow) {
  dfdb_table* t = q->t;
  const int64_t bs = t->block_size;
  const int64_t blk_row0 = ((int64_t)erow / bs) * bs;                          // first local row of the erroring block
  for (size_t k = 0; k < q->stages.size(); k++) {
    const Stage& st = q->stages[k];
    if (st.kind == ST_PRED) continue;
    if (k == 0) {
      // a leading range numbers table rows: blocks that end before its first element are skipped, blocks after its last are never read
      if (st.first() - (t->row_base + blk_row0) > bs) return false;         // _skip_if_can: elem.first - elem.offset > size_to_skip (the table's block size)
      if (st.last() <= t->row_base + blk_row0) return false;
      continue;
    }
    query_execute(q, (int)k);                                                  // survivors of stages [0, k): what stage k is fed
    if (st.last() <= st.stage_base + selected_before(q, blk_row0)) return false;
  }
  return true;
}
static void raise_reached_errors(dfdb_query* q, int nstages) {
  const uint64_t ew[3] = {q->err_row[0], q->err_row[1], q->err_row[2]};
  uint64_t er[3];
  for (int k = 0; k < 3; k++) er[k] = err_word_row(k, ew[k]);
  bool any_range = false;
  for (const Stage& st : q->stages) any_range = any_range || st.kind != ST_PRED;
  // in row order: the first error the iteration reaches is the one Julia throws; the parse word first, it wins a tie on the same row (first_error_kind)
  int order[3] = {2, 0, 1};
  std::stable_sort(order, order + 3, [&](int a, int b) { return er[a] < er[b]; });
  int raise = -1;
  if (!any_range) raise = order[0];                                           // every block is evaluated: the error of the smallest row
  else {
    q->err_checking = true;
    try {
      for (int i = 0; i < 3 && raise < 0; i++) { const int kind = order[i]; if (er[kind] != ~0ull && error_is_reached(q, er[kind])) raise = kind; }
      if (raise < 0) query_execute(q, nstages);                                // not reached: the result stands (the erroring rows are beyond the finish)
    } catch (...) { q->err_checking = false; throw; }
    q->err_checking = false;
  }
  q->err_row[0] = q->err_row[1] = q->err_row[2] = ~0ull;
  // (the row travels with the error: the shards of a multi-GPU group raise the error of the lowest GLOBAL row, group.cpp)
  if (raise == 0) { q->executed_stages = -1; throw Error(DFDB_ERR_DIVIDE, "DivideError: integer division error", (uint64_t)q->t->row_base + er[0]); }
  if (raise == 1) { q->executed_stages = -1; throw Error(DFDB_ERR_ARGUMENT, "InexactError: conversion is not exact", (uint64_t)q->t->row_base + er[1]); }
  if (raise == 2) { q->executed_stages = -1; throw_parse_error(ew[2], q->t->row_base); }
}

void query_execute(dfdb_query* q, int nstages) {
  ensure_state(q);
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx;
  if (nstages < 0 || nstages > (int)q->stages.size()) nstages = (int)q->stages.size();
  q->count = -1; q->prefix_valid = false; q->executed_stages = -1; q->cap_col = -1; q->cap_col2 = -1; q->cap_str_col = -1; q->agg_col = -1; q->const_str_col = -1;
  q->decoded_col = -1;
  q->comp_scanned.clear();
  for (auto& a : q->arenas) a.second.valid = false;      // the survivors' blocks of the previous selection
  q->gr_state = 0;             // a pending groupreduce belongs to the selection that is being replaced: its fetch must not restore the old one over this
  q->err_row[0] = q->err_row[1] = q->err_row[2] = ~0ull;
  // A range-like stage that is EMPTY (an empty range, an empty index vector) finishes the reference's iteration before the first block is read:
  // is_finished (selection.jl:192-196: `last <= offset` for ANY range stage of the queue) is tested ahead of every block (blocksiterator.jl:69-78).
  // Nothing is evaluated — a predicate of another stage that would raise DivideError on some row never runs (found by the fuzz soak: the engine raised).
  for (const Stage& st : q->stages) {
    const bool empty = (st.kind == ST_RANGE && st.n == 0) || ((st.kind == ST_INDICES || st.kind == ST_INTEGER) && st.idx.empty());
    if (!empty) continue;
    HIP_CHECK(hipMemsetAsync(q->bitmap.p, 0, padded_words(t->nrows) * 8, ctx->stream));
    HIP_CHECK(hipMemsetAsync(q->tile_counts.p, 0, (size_t)ceil_div(t->nrows, kTileRows) * 4, ctx->stream));
    scan_prefix(q);
    q->executed_stages = nstages;
    return;
  }
  if (nstages == 0) {
    LaunchTimer lt(ctx, "fill_ones");
    launch_fill_ones(ctx->stream, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), t->nrows);
  }
  for (int i = 0; i < nstages; i++) {
    const Stage& st = q->stages[(size_t)i];
    if (st.kind == ST_PRED) { run_predicate(q, *st.pred, i == 0, i + 1 == (int)q->stages.size()); q->prefix_valid = false; }
    else run_range(q, st, i == 0);
  }
  // A view that needs NO column at all — range-like stages only and a projection of constants — iterates nothing in the reference: BlocksIterator
  // opens one stream per required column and `isempty(it.streams)` ends the iteration before the first block (blocksiterator.jl:101,125).  Same here.
  if (nstages == (int)q->stages.size()) {
    std::vector<int> req;
    for (const Stage& st : q->stages) if (st.kind == ST_PRED) required_columns(*st.pred, req);
    for (const ProjCol& p : q->proj) required_columns(*p.expr, req);
    if (req.empty() && !q->proj.empty()) {
      HIP_CHECK(hipMemsetAsync(q->bitmap.p, 0, padded_words(t->nrows) * 8, ctx->stream));
      HIP_CHECK(hipMemsetAsync(q->tile_counts.p, 0, (size_t)ceil_div(t->nrows, kTileRows) * 4, ctx->stream));
    }
  }
  scan_prefix(q);
  q->executed_stages = nstages;
  if (!q->err_checking && (q->err_row[0] != ~0ull || q->err_row[1] != ~0ull || q->err_row[2] != ~0ull)) raise_reached_errors(q, nstages);
}

static void ensure_executed(dfdb_query* q) {
  if (q->executed_stages != (int)q->stages.size() || q->bitmap_rows != q->t->nrows) query_execute(q, -1);
}

int64_t query_count(dfdb_query* q, int nstages);
// ensure_executed for a consumer that hands results to the HOST (or builds on them: unique, groupreduce, a new column): an execution that decoded a column's
// resident LZ4 blocks on its way (decode_on_scan) is only as good as that decode, and the blocks' statuses are read — and a failed decode repeated once
// without the index — where query_count waits for the count (only dfdb_count did so).  Consumers that stay asynchronous on the device
// (dfdb_select_indices / _bitmap into device memory without a count, the group layer's device aggregates) are covered by the caller's next dfdb_count or
// dfdb_table_decode_status, as include/dfdb.h says.
void ensure_executed_checked(dfdb_query* q) {
  ensure_executed(q);
  if (q->decoded_col >= 0 || !q->comp_scanned.empty()) (void)query_count(q, -1);
}

int64_t query_count(dfdb_query* q, int nstages) {
  if (nstages < 0) { ensure_executed(q); if (q->count >= 0) return q->count; }
  else query_execute(q, nstages);
  dfdb_ctx* ctx = q->t->ctx;
  const int64_t ntiles = ceil_div(q->t->nrows, kTileRows);
  HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, q->prefix.as<uint64_t>() + ntiles, 8, hipMemcpyDeviceToHost, ctx->stream));
  stream_wait(ctx);
  int64_t n = ctx->pinned_scalar[0];
  // An execution that decoded a column's resident LZ4 blocks on its way (decode_on_scan) has results only as good as that decode: a block K7 gave
  // up on (a damaged copy, or err 9 — a sequence-start index that is not this stream's) leaves stale mask words, tile counts and column bytes
  // behind.  The statuses are read here, where the host waits for the count anyway.  A bad block drops the index
  // (table_decode_status); ONE more execution decodes by parsing and records a new one; bad again -> the blocks themselves are damaged.
  if (!q->comp_scanned.empty()) {
    // the same for the compressed-only columns this execution decoded inside its scan (several terms may have: each column's statuses are its last launch's)
    const std::vector<int> cols = q->comp_scanned;
    bool again = false;
    for (int col : cols) again = table_decode_status(q->t, col) > 0 || again;
    if (again) {
      query_execute(q, nstages < 0 ? -1 : nstages);
      for (int col : q->comp_scanned) {
        const int64_t bad = table_decode_status(q->t, col);
        if (bad > 0) { q->executed_stages = -1; fail(DFDB_ERR_FORMAT, "column %s: %lld of its resident LZ4 blocks do not decode", q->t->cols[(size_t)col].name.c_str(), (long long)bad); }
      }
      HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, q->prefix.as<uint64_t>() + ntiles, 8, hipMemcpyDeviceToHost, ctx->stream));
      stream_wait(ctx);
      n = ctx->pinned_scalar[0];
    }
  }
  if (q->decoded_col >= 0) {
    const int col = q->decoded_col;
    if (table_decode_status(q->t, col) > 0) {
      query_execute(q, nstages < 0 ? -1 : nstages);
      int64_t bad = q->decoded_col >= 0 ? table_decode_status(q->t, col) : 0;
      if (bad > 0) { q->executed_stages = -1; fail(DFDB_ERR_FORMAT, "column %s: %lld of its resident LZ4 blocks do not decode", q->t->cols[(size_t)col].name.c_str(), (long long)bad); }
      HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, q->prefix.as<uint64_t>() + ntiles, 8, hipMemcpyDeviceToHost, ctx->stream));
      stream_wait(ctx);
      n = ctx->pinned_scalar[0];
    }
  }
  if (nstages < 0) q->count = n;
  return n;
}

void query_select_bitmap(dfdb_query* q, uint64_t* out, int32_t memkind) {
  if (memkind == DFDB_MEM_DEVICE) ensure_executed(q); else ensure_executed_checked(q);
  hipStream_t s = q->t->ctx->stream;
  const size_t bytes = (size_t)ceil_div(q->t->nrows, 64) * 8;
  if (!bytes) return;
  HIP_CHECK(hipMemcpyAsync(out, q->bitmap.p, bytes, memkind == DFDB_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  if (memkind != DFDB_MEM_DEVICE) stream_wait(q->t->ctx);
}

void query_select_indices(dfdb_query* q, int64_t* out, int64_t cap, int32_t memkind, int64_t* n) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  ensure_executed(q);
  const int store = (int)ctx_option(ctx, "compact_store", kCompactStoreDefault);   // per context: two contexts may run different variants side by side
  static const char* const store_names[] = {"compact_indices.plain8", "compact_indices.nt8", "compact_indices.wt8", "compact_indices.nt16", "compact_indices.plain16",
                                            "compact_indices.nt16_lds4k", "compact_indices.plain16_lds4k"};
  prof_note(ctx, store_names[store >= 0 && store <= 6 ? store : 0]);
  const int gcap = 0;
  if (memkind == DFDB_MEM_DEVICE) {
    { LaunchTimer lt(ctx, "compact_indices");
      launch_compact_indices(s, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), out, t->nrows, t->row_base, cap, store, gcap); }
    if (n) *n = query_count(q, -1);
    return;
  }
  const int64_t cnt = query_count(q, -1);
  if (n) *n = cnt;
  const int64_t m = std::min(cnt, cap);
  if (m <= 0) return;
  q->tmp_b.ensure((size_t)m * 8);
  { LaunchTimer lt(ctx, "compact_indices");
    launch_compact_indices(s, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), q->tmp_b.as<int64_t>(), t->nrows, t->row_base, m, store, gcap); }
  HIP_CHECK(hipMemcpyAsync(out, q->tmp_b.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
  stream_wait(q->t->ctx);
}

// ---------------------------------------------------------------- compressed-only projection columns
// The source pointer of a gather over a fixed-width column.  A compressed-only column (keep_compressed = 2) has no decoded array: the blocks of the current
// selection that KEPT A ROW are decoded into an arena this query owns — at their natural offsets inside the span [first such block, last such block], so the
// gather kernels address it like the column itself through a shifted base — and the others are never touched (blocksiterator.jl:111-113: a block with an
// empty selection skips its projection columns).  Synchronises (the survivors per block are read on the host, like the reference's loop reads them).
static const void* gather_source(dfdb_query* q, int ord) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  Column& c = t->cols[(size_t)ord];
  if (!c.comp_only || c.data.p) return c.data.p;
  const int w = dt_width(c.dtype);
  dfdb_query::Arena& a = q->arenas[ord];
  if (!a.valid || a.from != c.comp.p) {                  // (a column that was loaded or compressed again since: other blocks)
    a.from = c.comp.p;
    std::vector<int64_t> counts;
    query_block_counts(q, t->block_size, counts);
    int64_t first = -1, last = -1;
    std::vector<Lz4Block> sub;
    for (int64_t b = 0; b < (int64_t)counts.size() && b < c.comp_nblocks; b++) if (counts[(size_t)b] > 0) { if (first < 0) first = b; last = b; }
    a.first_row = first < 0 ? 0 : first * t->block_size; a.nblocks = 0;
    if (first >= 0) {
      const int64_t base_off = c.comp_blocks_host[(size_t)first].dst_off;
      for (int64_t b = first; b <= last; b++) if (counts[(size_t)b] > 0) { Lz4Block x = c.comp_blocks_host[(size_t)b]; x.dst_off -= base_off; sub.push_back(x); }
      const Lz4Block& lb = c.comp_blocks_host[(size_t)last];
      a.buf.ensure((size_t)(lb.dst_off - base_off) + (size_t)lb.dst_len + 256);
      a.blocks.ensure(sub.size() * sizeof(Lz4Block)); a.status.ensure(sub.size() * 4);
      HIP_CHECK(hipMemcpyAsync(a.blocks.p, sub.data(), sub.size() * sizeof(Lz4Block), hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemsetAsync(a.status.p, 0, sub.size() * 4, s));
      const int pipe = (int)ctx_option(ctx, "lz4_pipeline", -1);
      const int mode = column_lz4_index(ctx, c, lz4_decode_takes_index((int32_t)sub.size(), pipe));
      { LaunchTimer lt(ctx, "lz4_decode");
        prof_note(ctx, "lz4_decode.survivors");
        launch_lz4_decode(s, c.comp.as<uint8_t>(), a.buf.as<uint8_t>(), a.blocks.as<Lz4Block>(), (int32_t)sub.size(), a.status.as<int32_t>(), pipe, c.comp_index.as<uint32_t>(),
                          mode == 1 ? 0 : mode); }      // (a subset of the blocks cannot RECORD the column's index)
      if (mode == 1) c.comp_index_state = 0;
      std::vector<int32_t> st(sub.size());
      HIP_CHECK(hipMemcpyAsync(st.data(), a.status.p, st.size() * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));            // (also: `sub` is pageable host memory)
      int64_t bad = 0; for (int32_t v : st) bad += v != 0;
      if (bad && mode == 2) {                        // the index may be what is damaged: once more by parsing
        HIP_CHECK(hipMemsetAsync(a.status.p, 0, sub.size() * 4, s));
        launch_lz4_decode(s, c.comp.as<uint8_t>(), a.buf.as<uint8_t>(), a.blocks.as<Lz4Block>(), (int32_t)sub.size(), a.status.as<int32_t>(), pipe, nullptr, 0);
        HIP_CHECK(hipMemcpyAsync(st.data(), a.status.p, st.size() * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        bad = 0; for (int32_t v : st) bad += v != 0;
        if (!bad) { c.comp_index.release(); c.comp_index_state = 0; }
      }
      if (bad) fail(DFDB_ERR_FORMAT, "column %s: %lld of its resident LZ4 blocks do not decode", c.name.c_str(), (long long)bad);
      a.nblocks = (int64_t)sub.size();
    } else a.buf.ensure(256);
    a.valid = true;
  }
  // row r of the column lives at arena byte (r - first_row) * w: hand the kernels the base that makes `src + r * w` land there (never dereferenced below first_row)
  return (const void*)(a.buf.as<uint8_t>() - (intptr_t)a.first_row * w);
}

// ---------------------------------------------------------------- materialize
static bool string_captured(const dfdb_query* q, const Column& col) {
  return q->cap_str_col >= 0 && &q->t->cols[(size_t)q->cap_str_col] == &col && q->executed_stages == (int)q->stages.size();
}

// selected string bytes per 1024-row tile -> exclusive scan (output arena offsets); returns total
static int64_t string_out_offsets(dfdb_query* q, const Column& col, DevBuf& out_sizes_tmp, int32_t* out_sizes, int64_t cap, DevBuf& tile_off_out) {
  dfdb_ctx* ctx = q->t->ctx; hipStream_t s = ctx->stream;
  const int64_t nct = ceil_div(q->t->nrows, kTileRows);
  DevBuf& tb = q->tmp_c; tb.ensure((size_t)(nct + 8) * 4);
  tile_off_out.ensure((size_t)(nct + 8) * 8);
  DevBuf& scratch = q->str_scratch; scratch.ensure(scan_counts_scratch_bytes(nct));
  int32_t* dst_sizes = out_sizes;
  if (!dst_sizes) { out_sizes_tmp.ensure((size_t)std::max<int64_t>(cap, 1) * 4); dst_sizes = out_sizes_tmp.as<int32_t>(); }
  if (col.dict_n > 0) {
    // K9: the selected rows' codes, compacted by K3 (kept in q->dict_sel for the bytes pass), then sizes and byte totals per 1024 OUTPUT rows
    const int64_t n = std::min<int64_t>(cap, query_count(q, -1));
    const int64_t not_ = ceil_div(std::max<int64_t>(n, 1), kTileRows);
    q->dict_sel.ensure((size_t)std::max<int64_t>(n, 1) * 2 + 256);
    { LaunchTimer lt(ctx, "gather"); launch_gather(s, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), col.dict_codes.p, q->dict_sel.p, 2, q->t->nrows, n); }
    DevBuf& otb = q->tmp_c; otb.ensure((size_t)(not_ + 8) * 4);
    tile_off_out.ensure((size_t)(not_ + 8) * 8);
    scratch.ensure(scan_counts_scratch_bytes(not_));
    HIP_CHECK(hipMemsetAsync(otb.p, 0, (size_t)(not_ + 8) * 4, s));
    { LaunchTimer lt(ctx, "dict_expand_sizes"); launch_dict_expand_sizes(s, q->dict_sel.as<uint16_t>(), n, col.dict_len.as<int32_t>(), dst_sizes, otb.as<uint32_t>()); }
    launch_scan_counts(s, otb.as<uint32_t>(), tile_off_out.as<uint64_t>(), not_, scratch.as<uint64_t>());
    HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar + 1, tile_off_out.as<uint64_t>() + not_, 8, hipMemcpyDeviceToHost, s));
    stream_wait(q->t->ctx);
    return ctx->pinned_scalar[1];
  }
  if (string_captured(q, col)) {     // K5 kept the selected rows: their byte totals per tile are already there
    launch_scan_counts(s, q->cap_str_tb.as<uint32_t>(), tile_off_out.as<uint64_t>(), nct, scratch.as<uint64_t>());
    HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar + 1, tile_off_out.as<uint64_t>() + nct, 8, hipMemcpyDeviceToHost, s));
    stream_wait(q->t->ctx);
    return ctx->pinned_scalar[1];
  }
  { LaunchTimer lt(ctx, "str_gather_sizes");
    launch_str_gather_sizes(s, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), col.data.as<int32_t>(), dst_sizes, tb.as<uint32_t>(), q->t->nrows, cap); }
  launch_scan_counts(s, tb.as<uint32_t>(), tile_off_out.as<uint64_t>(), nct, scratch.as<uint64_t>());
  HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar + 1, tile_off_out.as<uint64_t>() + nct, 8, hipMemcpyDeviceToHost, s));
  stream_wait(q->t->ctx);
  return ctx->pinned_scalar[1];
}

int64_t query_string_bytes(dfdb_query* q, int i) {
  ensure_executed_checked(q);
  if (i < 0 || (size_t)i >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", i);
  const Node& e = *q->proj[(size_t)i].expr;
  if (dt_base(e.dtype) != DFDB_STRING) return 0;
  if (e.op != DFIR_COL) fail(DFDB_ERR_UNSUPPORTED, "computed String columns are outside the IR");
  const Column& col = need_resident(q->t, e.col);
  const int64_t cnt = query_count(q, -1);
  if (q->const_str_col == e.col && q->executed_stages == (int)q->stages.size()) return cnt * (int64_t)q->const_str.size();
  return string_out_offsets(q, col, q->str_sizes, nullptr, cnt, q->str_toff);
}

// one output column of the projection (ProjectionExecutor.eval_on_range for column p: projection.jl:128-154)
void materialize_col(dfdb_query* q, int32_t p, dfdb_outcol& o, int64_t cnt) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const Node& e = *q->proj[(size_t)p].expr;
  o.dtype = e.dtype; o.count = cnt; o.nbytes = 0;
  const bool dev = o.memkind == DFDB_MEM_DEVICE;
  const int w = dt_width(e.dtype);
  if (cnt == 0) return;
  if (!o.data) fail(DFDB_ERR_ARGUMENT, "output column %d has no data buffer", p);
  if (e.op == DFIR_COL) {   // ColProjExec: buffer .= data[name][range] (projection.jl:130-133)
    const void* gsrc = nullptr;
    if (t->cols[(size_t)e.col].comp_only && !dt_nullable(e.dtype) && dt_base(e.dtype) != DFDB_STRING) {
      if (!t->cols[(size_t)e.col].resident) fail(DFDB_ERR_ARGUMENT, "column %s is not resident on the device (dfdb_table_load it first)", t->cols[(size_t)e.col].name.c_str());
      gsrc = gather_source(q, e.col);        // compressed-only: the blocks with survivors, decoded for this query (no whole-column decode)
    }
    const Column& col = gsrc ? t->cols[(size_t)e.col] : need_resident(t, e.col);
    if (!gsrc) gsrc = col.data.p;
    if (dt_base(e.dtype) == DFDB_STRING) {   // FlatStringsVector gather (FlatStringsVectors.jl:136-157)
      if (q->const_str_col == e.col && q->executed_stages == (int)q->stages.size()) {   // every selected row holds q->const_str (run_predicate)
        const int64_t plen = (int64_t)q->const_str.size(), total = cnt * plen;
        o.nbytes = total;
        if (total > o.bytes_cap) fail(DFDB_ERR_ARGUMENT, "output column %d needs %lld string bytes, capacity is %lld", p, (long long)total, (long long)o.bytes_cap);
        DevBuf &csz = q->str_sizes, &cby = q->str_bytes;
        int32_t* d_sizes = dev ? (int32_t*)o.data : (csz.ensure((size_t)cnt * 4), csz.as<int32_t>());
        uint8_t* d_bytes = dev ? o.bytes : (cby.ensure((size_t)total + 64), cby.as<uint8_t>());
        DevBuf& pb = q->tmp_a; pb.ensure((size_t)plen + 64);
        if (plen) { HIP_CHECK(hipMemcpyAsync(pb.p, q->const_str.data(), (size_t)plen, hipMemcpyHostToDevice, s)); stream_wait(ctx); }
        { LaunchTimer lt(ctx, "fill_const_strings"); launch_fill_const_strings(s, d_sizes, d_bytes, cnt, pb.as<uint8_t>(), (int32_t)plen); }
        if (!dev) {
          HIP_CHECK(hipMemcpyAsync(o.data, d_sizes, (size_t)cnt * 4, hipMemcpyDeviceToHost, s));
          if (total > 0) HIP_CHECK(hipMemcpyAsync(o.bytes, d_bytes, (size_t)total, hipMemcpyDeviceToHost, s));
          stream_wait(ctx);
        }
        return;
      }
      DevBuf &dsz = q->str_sizes, &toff = q->str_toff, &dbytes = q->str_bytes;   // reused across calls (hipFree would sync the device)
      int32_t* d_sizes = dev ? (int32_t*)o.data : nullptr;
      const int64_t total = string_out_offsets(q, col, dsz, d_sizes, cnt, toff);
      if (!d_sizes) d_sizes = dsz.as<int32_t>();
      o.nbytes = total;
      if (total > o.bytes_cap) fail(DFDB_ERR_ARGUMENT, "output column %d needs %lld string bytes, capacity is %lld", p, (long long)total, (long long)o.bytes_cap);
      uint8_t* d_bytes = dev ? o.bytes : nullptr;
      if (!dev) { dbytes.ensure((size_t)total + 64); d_bytes = dbytes.as<uint8_t>(); }
      if (col.dict_n > 0) {              // K9: the compacted codes of string_out_offsets -> bytes out of the dictionary
        if (total > 0) {
          LaunchTimer lt(ctx, "dict_expand_bytes");
          launch_dict_expand_bytes(s, q->dict_sel.as<uint16_t>(), cnt, col.dict_len.as<int32_t>(), col.dict_off.as<uint32_t>(), col.dict_bytes.as<uint8_t>(), toff.as<uint64_t>(), d_bytes, total);
        }
      } else if (string_captured(q, col)) {     // sizes and bytes: one contiguous copy per tile out of the match pass's capture
        LaunchTimer lt(ctx, "str_compact_captured");
        const StrCapture sc{q->cap_str_sizes.as<int32_t>(), q->cap_str_bytes.as<uint8_t>(), q->cap_str_tb.as<uint32_t>()};
        launch_str_compact_captured(s, sc, q->prefix.as<uint64_t>(), (const int64_t*)col.tile_off.p, toff.as<uint64_t>(), d_sizes, d_bytes, t->nrows, cnt, total);
      } else if (total > 0) {
        LaunchTimer lt(ctx, "str_gather_bytes");
        launch_str_gather_bytes(s, q->bitmap.as<uint64_t>(), col.data.as<int32_t>(), (const int64_t*)col.tile_off.p, col.bytes.as<uint8_t>(),
                                toff.as<uint64_t>(), d_bytes, t->nrows, total);
      }
      if (!dev) {
        HIP_CHECK(hipMemcpyAsync(o.data, d_sizes, (size_t)cnt * 4, hipMemcpyDeviceToHost, s));
        if (total > 0) HIP_CHECK(hipMemcpyAsync(o.bytes, d_bytes, (size_t)total, hipMemcpyDeviceToHost, s));
        stream_wait(ctx);
      }
      return;
    }
    DevBuf stage; void* dst = o.data;
    if (!dev) { stage.ensure((size_t)cnt * w); dst = stage.p; }
    if ((q->cap_col == e.col || q->cap_col2 == e.col) && w == 8 && q->executed_stages == (int)q->stages.size()) {   // the scan kept these values: contiguous copy per tile
      LaunchTimer lt(ctx, "compact_captured");
      launch_compact_captured(s, (q->cap_col == e.col ? q->cap_buf : q->cap_buf2).as<uint64_t>(), q->prefix.as<uint64_t>(), (uint64_t*)dst, t->nrows, cnt);
    } else {
      LaunchTimer lt(ctx, "gather");
      launch_gather(s, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), gsrc, dst, w, t->nrows, cnt);
    }
    if (!dev) HIP_CHECK(hipMemcpyAsync(o.data, dst, (size_t)cnt * w, hipMemcpyDeviceToHost, s));
    if (dt_nullable(e.dtype) && o.missing) {
      DevBuf ms; uint8_t* md = o.missing;
      if (!dev) { ms.ensure((size_t)cnt); md = ms.as<uint8_t>(); }
      launch_gather_bits(s, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), col.missing.as<uint64_t>(), md, t->nrows, cnt);
      if (!dev) { HIP_CHECK(hipMemcpyAsync(o.missing, md, (size_t)cnt, hipMemcpyDeviceToHost, s)); stream_wait(ctx); }
    }
    if (!dev) stream_wait(ctx);   // staging buffers die at scope exit; device outputs stay stream-ordered, no host wait
  } else {                  // BroadcastExecutor: computed column (projection.jl:128-129)
    if (dt_base(e.dtype) == DFDB_STRING) fail(DFDB_ERR_UNSUPPORTED, "computed String columns are outside the IR");
    DevBuf stage, mstage; void* dst = o.data;
    if (!dev) { stage.ensure((size_t)cnt * w); dst = stage.p; }
    uint8_t* mdst = nullptr;                               // Union{R,Missing} result: one flag byte per selected row
    if (dt_nullable(e.dtype) && o.missing) { mdst = o.missing; if (!dev) { mstage.ensure((size_t)cnt); mdst = mstage.as<uint8_t>(); } }
    // a transform of ONE plain column (rem / col * k + d / col / k: expr.cpp match_column_transform) rides on the gather of that column
    ScanTerm tf; const Node* tcol = nullptr;
    if (w == 8 && !dt_nullable(e.dtype) && match_column_transform(&e, tf, tcol) && tf.pre != 0 && !dt_nullable(tcol->dtype) && t->cols[(size_t)tcol->col].resident) {
      const Column& sc = t->cols[(size_t)tcol->col];
      if ((q->cap_col == tcol->col || q->cap_col2 == tcol->col) && dt_width(sc.dtype) == 8 && q->executed_stages == (int)q->stages.size()) {
        LaunchTimer lt(ctx, "compact_captured");                  // the scan kept the column's selected values: the transform rides on the copy
        launch_compact_captured_transform(s, (q->cap_col == tcol->col ? q->cap_buf : q->cap_buf2).as<uint64_t>(), q->prefix.as<uint64_t>(), dt_base(sc.dtype), tf, (uint64_t*)dst, t->nrows, cnt);
      } else {
        LaunchTimer lt(ctx, "gather");
        launch_gather_transform(s, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), gather_source(q, tcol->col), dt_base(sc.dtype), tf, dst, t->nrows, cnt);
      }
    } else if (e.op == DFIR_CAST && e.a->op == DFIR_COL && dt_base(e.a->dtype) == DFDB_STRING && ctx_option(ctx, "parse_kernel", 1) != 0)
      run_str_parse(q, e, dst, cnt);                        // exactly parse.(T, s): the conversion kernel (k_parse.hip); "parse_kernel" = 0: the interpreter
    else
    run_interp_project(q, e, dst, cnt, mdst);
    if (!dev) {
      HIP_CHECK(hipMemcpyAsync(o.data, dst, (size_t)cnt * w, hipMemcpyDeviceToHost, s));
      if (mdst) HIP_CHECK(hipMemcpyAsync(o.missing, mdst, (size_t)cnt, hipMemcpyDeviceToHost, s));
      stream_wait(ctx);
    }
  }
}

void query_materialize(dfdb_query* q, dfdb_outcol* outs, int32_t ncols) {
  ensure_executed(q);
  if (ncols != (int32_t)q->proj.size()) fail(DFDB_ERR_ARGUMENT, "ArgumentError: view has %zu columns, %d outputs given", q->proj.size(), ncols);
  const int64_t cnt = query_count(q, -1);
  // a computed column that raises (DivideError / InexactError on a selected row): the reference evaluates block by block and, inside a block, the projection's
  // columns in order (projection.jl:149-154 under blocksiterator.jl:98-121) — the error it throws is the one of the first BLOCK that holds an erroring row, the
  // first such COLUMN in that block, the first such row of that column.  The columns are computed whole here, so their first erroring rows are collected and
  // the choice is made at the end.
  uint64_t pe[3], best_block = ~0ull, best_word = ~0ull; int best_kind = -1;
  const uint64_t bs = (uint64_t)std::max<int64_t>(q->t->block_size, 1);
  q->proj_err = pe;
  try {
    for (int32_t p = 0; p < ncols; p++) {
      pe[0] = pe[1] = pe[2] = ~0ull;
      materialize_col(q, p, outs[p], cnt);
      const int k = first_error_kind(pe);
      const uint64_t r = k < 0 ? ~0ull : err_word_row(k, pe[k]);
      if (r != ~0ull && r / bs < best_block) { best_block = r / bs; best_kind = k; best_word = pe[k]; }
    }
  } catch (...) { q->proj_err = nullptr; throw; }
  q->proj_err = nullptr;
  if (best_kind == 0) fail(DFDB_ERR_DIVIDE, "DivideError: integer division error");
  if (best_kind == 1) fail(DFDB_ERR_ARGUMENT, "InexactError: conversion is not exact");
  if (best_kind == 2) throw_parse_error(best_word, q->t->row_base);
}

// add_column!(table, name, lazy_col) (src/tables/table.jl:96-124): the p-th column of the view materialised into a new
// RESIDENT column of dst without leaving the device.  dst may be the view's own table (then every row must be selected).
void launch_pack_flags(hipStream_t s, const uint8_t* flags, uint64_t* bits, int64_t n);
void table_add_from_query(dfdb_table* dst, const char* name, dfdb_query* q, int32_t p) {
  const bool ooc = query_out_of_core(q);      // the view's columns are not resident: the new column is made from the block stream (csrc/ooc.cpp), chunk by chunk
  if (!ooc) ensure_executed_checked(q);
  if (p < 0 || (size_t)p >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", p);
  if (dst->ctx != q->t->ctx) fail(DFDB_ERR_ARGUMENT, "the destination table lives on another context");
  for (auto& c : dst->cols) if (c.name == name) fail(DFDB_ERR_ARGUMENT, "ArgumentError: Duplicated column %s", name);
  const Node& e = *q->proj[(size_t)p].expr;
  const int64_t cnt = ooc ? ooc_count(q) : query_count(q, -1);
  if (dst->nrows >= 0 && dst->nrows != cnt)
    fail(DFDB_ERR_ARGUMENT, "ArgumentError: column has %lld rows but the table has %lld", (long long)cnt, (long long)dst->nrows);
  dfdb_ctx* ctx = dst->ctx; hipStream_t s = ctx->stream;
  Column c; c.name = name; c.dtype = e.dtype; c.id = 1; c.nrows = cnt;
  if (e.op == DFIR_COL) c.logical = q->t->cols[(size_t)e.col].logical;   // a projected Date / DateTime / Char column keeps its type
  for (auto& o : dst->cols) c.id = std::max(c.id, o.id + 1);
  dfdb_outcol o{}; o.memkind = DFDB_MEM_DEVICE;
  DevBuf flags;
  if (dt_base(e.dtype) == DFDB_STRING) {
    const int64_t total = ooc ? ooc_string_bytes(q, p) : query_string_bytes(q, p);
    c.data.ensure((size_t)cnt * 4 + 256);
    c.nbytes = total; c.bytes.ensure((size_t)total + 64);
    HIP_CHECK(hipMemsetAsync((char*)c.bytes.p + total, 0, 64, s));
    o.data = c.data.p; o.bytes = c.bytes.as<uint8_t>(); o.bytes_cap = total;
  } else {
    c.data.ensure((size_t)cnt * dt_width(e.dtype) + 256);
    o.data = c.data.p;
    if (dt_nullable(e.dtype)) { flags.ensure((size_t)cnt + 64); HIP_CHECK(hipMemsetAsync(flags.p, 0, (size_t)cnt + 64, s)); o.missing = flags.as<uint8_t>(); }
  }
  if (ooc) ooc_materialize_column(q, p, &o); else materialize_col(q, p, o, cnt);
  if (dt_base(e.dtype) == DFDB_STRING) set_string_tile_offsets(ctx, c);
  else if (dt_nullable(e.dtype)) {
    const size_t nw = (size_t)(round_up(cnt > 0 ? cnt : 1, kCTileRows) / 64 + 64);
    c.missing.ensure(nw * 8);
    HIP_CHECK(hipMemsetAsync(c.missing.p, 0, nw * 8, s));
    if (cnt) launch_pack_flags(s, flags.as<uint8_t>(), c.missing.as<uint64_t>(), cnt);
  }
  HIP_CHECK(hipStreamSynchronize(s));
  c.resident = true;
  if (dst->nrows < 0) dst->nrows = cnt;
  dst->cols.push_back(std::move(c));
}

// the device half of an aggregate: leaves {value, selected count} (16 bytes) of sum / min / max over projection column i in
// q->red_result on the engine stream and returns the accumulator dtype (DFDB_I64 / DFDB_U64 / DFDB_F64).  No host wait: the group
// layer (group.cpp) hands the 16 bytes to the RCCL all-reduce as they are; an empty selection leaves the identity of `op`.
int query_aggregate_device(dfdb_query* q, int32_t op, int32_t i) {
  ensure_executed(q);
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  if (i < 0 || (size_t)i >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", i);
  const Node& e = *q->proj[(size_t)i].expr;
  if (!dt_isnum(e.dtype) || dt_nullable(e.dtype)) fail(DFDB_ERR_UNSUPPORTED, "aggregate over %s is not supported", dt_name(e.dtype).c_str());
  int dt = dt_base(e.dtype);
  q->red_scratch.ensure(reduce_scratch_bytes()); q->red_result.ensure(64);
  if (op == q->agg_op && e.op == DFIR_COL && q->agg_col == e.col && q->executed_stages == (int)q->stages.size()) {
    // the scan already reduced the selected values of this column per tile (k_scan_terms EXTRA = 2 / 3 / 4): reduce the partials
    const int64_t nt = ceil_div(t->nrows, kTileRows);
    if (q->agg_ones_tiles != nt) {
      q->agg_ones.ensure(padded_words(nt) * 8);
      HIP_CHECK(hipMemsetAsync(q->agg_ones.p, 0xff, (size_t)(nt / 64) * 8, s));
      const uint64_t tail = (nt & 63) ? ((1ull << (nt & 63)) - 1ull) : 0ull;
      HIP_CHECK(hipMemcpyAsync((uint64_t*)q->agg_ones.p + nt / 64, &tail, 8, hipMemcpyHostToDevice, s));
      stream_wait(ctx);
      q->agg_ones_tiles = nt;
    }
    dt = q->agg_dtype == DFDB_F64 ? DFDB_F64 : (q->agg_dtype == DFDB_U64 ? DFDB_U64 : DFDB_I64);
    { LaunchTimer lt(ctx, "reduce_partials"); launch_reduce(s, q->agg_ones.as<uint64_t>(), q->agg_partials.p, dt, op, nt, q->red_scratch.p, q->red_result.p); }
    // the count slot of the partial reduce counts TILES: the selected rows are the scan total
    HIP_CHECK(hipMemcpyAsync((uint64_t*)q->red_result.p + 1, q->prefix.as<uint64_t>() + nt, 8, hipMemcpyDeviceToDevice, s));
  } else if (e.op == DFIR_COL) {
    { LaunchTimer lt(ctx, "reduce"); launch_reduce(s, q->bitmap.as<uint64_t>(), need_resident(t, e.col).data.p, dt, op, t->nrows, q->red_scratch.p, q->red_result.p); }
  } else {   // computed column: materialise the selected values, then reduce them all
    const int64_t cnt = query_count(q, -1);
    DevBuf &full = q->tmp_b, &ones = q->tmp_c;
    full.ensure((size_t)std::max<int64_t>(cnt, 1) * dt_width(dt) + 256);
    if (cnt) run_interp_project(q, e, full.p, cnt, nullptr);
    const size_t nw = padded_words(cnt);
    ones.ensure(nw * 8);
    HIP_CHECK(hipMemsetAsync(ones.p, 0xff, (size_t)(cnt / 64) * 8, s));
    uint64_t tail = (cnt & 63) ? ((1ull << (cnt & 63)) - 1ull) : 0ull;
    HIP_CHECK(hipMemcpyAsync((uint64_t*)ones.p + cnt / 64, &tail, 8, hipMemcpyHostToDevice, s));
    stream_wait(q->t->ctx);
    { LaunchTimer lt(ctx, "reduce"); launch_reduce(s, ones.as<uint64_t>(), full.p, dt, op, cnt, q->red_scratch.p, q->red_result.p); }
  }
  return dt_isfloat(dt) ? DFDB_F64 : (dt == DFDB_U64 ? DFDB_U64 : DFDB_I64);
}

void query_aggregate(dfdb_query* q, int32_t op, int32_t i, int64_t* out_i, double* out_f) {
  if (op == DFDB_AGG_COUNT) { const int64_t n = query_count(q, -1); if (out_i) *out_i = n; if (out_f) *out_f = (double)n; return; }
  ensure_executed_checked(q);                       // (a host-facing result: a decode_on_scan execution answers for its decode first)
  const int dt = query_aggregate_device(q, op, i);
  dfdb_ctx* ctx = q->t->ctx;
  HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, q->red_result.p, 16, hipMemcpyDeviceToHost, ctx->stream));
  stream_wait(ctx);
  if (ctx->pinned_scalar[1] == 0 && op != DFDB_AGG_SUM) fail(DFDB_ERR_ARGUMENT, "ArgumentError: reducing over an empty collection is not allowed");
  if (dt == DFDB_F64) { double d; memcpy(&d, &ctx->pinned_scalar[0], 8); if (out_f) *out_f = d; if (out_i) *out_i = (int64_t)d; }
  else { const int64_t v = ctx->pinned_scalar[0]; if (out_i) *out_i = v; if (out_f) *out_f = dt == DFDB_U64 ? (double)(uint64_t)v : (double)v; }
}

}  // namespace dfdb
