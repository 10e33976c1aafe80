// query.cpp — the selection side of a DFView on the device: SelectionQueue composition, stage execution (a predicate stage is planned, then run),
// the placement calibration, count, bitmap, indices.  What is made of the selected rows — materialize, aggregates — is project.cpp.
//
// Replaces (paths in the reference tree): SelectionQueue add/_new_queue src/tables/selection.jl:37-60,
// SelectionExecutor.apply :161-167 with its range :94-111 and predicate :133-157 stages, the block loop of
// src/io/blocksiterator.jl:98-145, nrow src/tables/view.jl:192-206.
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

namespace dfdb {

// the launcher living in k_interp.hip that takes an engine-level description
void run_interp_predicate(dfdb_query* q, const Node& pred, bool and_existing);

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
// against a few candidate bitmap allocations spread over free HBM and the fastest stays with the column.  Queries that scan the column borrow it (one
// at a time; others use their own).  ctx option "placement_calibrate" = 1 asks for it (default 0).  One-time cost per column: 27 scans (~35 ms per 1e9
// rows) plus the candidates' allocation, 0.03-1.4 s measured (profiles/r2_placement_cost.txt) — worth it for a column that stays resident and is scanned
// thousands of times, not for a short session, which is why it is opt-in; stream slots never calibrate.
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
    const int kCand = 8;                    // candidate bitmaps
    if (free_b < (size_t)kCand * bytes + ((size_t)4 << 30)) return;      // not enough room to look around: keep the query's own
    std::vector<DevBuf> cand((size_t)kCand);
    try {
      for (int k = 0; k < kCand; k++) cand[(size_t)k].ensure(bytes);
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
    if (kCol > 0 && dt_base(c.dtype) != DFDB_STRING && c.data.bytes > 0 && free_b > (size_t)(kCol + 1) * c.data.bytes + (size_t)kCand * bytes + ((size_t)8 << 30)) {
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
    // of six processes: 1.195-1.236 ms), the search costs four 4-MB allocations and 3 scans each
    const int kTc = 4;
    if (q->tile_counts.bytes > 0) {
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
    HIP_CHECK(hipStreamSynchronize(s));                 // the candidates die here
    HIP_CHECK(hipMemsetAsync(q->bitmap.p, 0, bytes, s));
    cand.clear();                                       // (freed inside the timed span)
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
  launch_dict_pair(s, DictSide{ca.dict_codes.as<uint16_t>(), rb.as<uint32_t>(), (int32_t)na}, DictSide{cb.dict_codes.as<uint16_t>(), rb.as<uint32_t>() + na, (int32_t)nb}, op,
                   q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), q->t->nrows, have);
}

// ---------------------------------------------------------------- predicate stage: plan, then run
// A predicate stage is the AND of its conjuncts, each routed to the cheapest kernel that is exact for it.  plan_predicate decides everything before the
// first launch — the kind of every conjunct, the dictionary look-up tables, what the last term batch does besides its mask — and run_plan launches the
// steps in one fixed order: interpreter, dictionary LUT scans, string matches, string pairs, missing masks, OR batches, compressed-only scans, term batches.
struct DictLutStep { int ord; std::vector<uint32_t> lut; };           // a Boolean function of ONE dictionary column's entry: one bit per entry
struct StrStep { int ord, mode; std::string pat; std::vector<uint32_t> lut; };   // k_strings.hip's modes; lut: the column has a dictionary (K9), else empty
struct PairStep { int a, b, op; };                                    // s1 OP s2 over two String columns
struct MissStep { const uint64_t* bits; bool negate; };               // a nullable fixed-width column's missing bitmap as the mask
struct CompStep { ScanTerm tm; int ord; };                            // a simple term the decoder evaluates over a compressed-only column
struct TermBatch { ScanTerms terms; int ords[kMaxTerms]; };           // up to kMaxTerms AND-ed simple terms, the table ordinal of each beside it
struct PredPlan {
  const Node* interp = nullptr;      // the generic conjuncts as ONE program over `c1 & c2 & ...` (interp_owned holds the AND of several)
  NodePtr interp_owned;
  std::vector<DictLutStep> dict_luts;
  std::vector<StrStep> strs;
  std::vector<PairStep> pairs;
  std::vector<MissStep> miss;
  std::vector<ScanTerms> or_batches; // a conjunct that is itself a disjunction of simple terms — (a > c1) | (x < c2) — is one k_scan_terms pass with combine_or
  std::vector<CompStep> comp_terms;
  std::vector<TermBatch> term_batches;
  int extra = EX_NONE;               // what the LAST term batch does with its last term (and, EX_CAPTURE2, the one before it): plan_rider
  bool str_capture = false;          // the one string match of this plan keeps the selected rows' sizes and bytes (K5 CAP)
  size_t steps() const {
    return (interp ? 1 : 0) + dict_luts.size() + strs.size() + pairs.size() + miss.size() + or_batches.size() + comp_terms.size() + term_batches.size();
  }
};
static bool ex_captures(int ex) { return ex == EX_CAPTURE || ex == EX_CAPTURE2; }
static bool ex_reduces(int ex) { return ex == EX_SUM || ex == EX_MIN || ex == EX_MAX; }

static bool push_or_term(dfdb_table* t, const Node& n, ScanTerms& out) {
  ScanTerm tm; int ord;
  if (out.n == kMaxTerms || !match_simple_term(n, *t, tm, ord)) return false;
  tm.col = need_resident(t, ord).data.p;
  out.t[out.n++] = tm;
  return true;
}
static bool match_or(dfdb_table* t, const Node& n, ScanTerms& out) {
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
        if (!push_or_term(t, eq, out)) return false;
      }
      continue;
    }
    if (!push_or_term(t, *l, out)) return false;
  }
  return out.n >= 2;
}
// a disjunction (and negations) of string terms over ONE dictionary column — (brand == "sony") | (brand == "apple"), !startswith(brand, "x") — is a
// Boolean function of the dictionary entry: one bit-table lookup of the codes instead of string compares in the interpreter
static bool dict_only(const dfdb_table* t, const Node& n, int& ord) {
  if ((n.op == DFIR_OR || n.op == DFIR_AND || n.op == DFIR_XOR) && n.a && n.b) return dict_only(t, *n.a, ord) && dict_only(t, *n.b, ord);
  if (n.op == DFIR_NOT && n.a) return dict_only(t, *n.a, ord);
  int o, mode; std::string pat;
  if (!match_string_term(n, *t, o, mode, pat)) return false;
  if (ord >= 0 && o != ord) return false;
  if (t->cols[(size_t)o].dict_n <= 0 || !t->cols[(size_t)o].resident) return false;
  ord = o; return true;
}
static bool dict_eval(const dfdb_table* t, const Node& n, const std::string& e) {
  if (n.op == DFIR_OR) return dict_eval(t, *n.a, e) || dict_eval(t, *n.b, e);
  if (n.op == DFIR_AND) return dict_eval(t, *n.a, e) && dict_eval(t, *n.b, e);
  if (n.op == DFIR_XOR) return dict_eval(t, *n.a, e) != dict_eval(t, *n.b, e);
  if (n.op == DFIR_NOT) return !dict_eval(t, *n.a, e);
  int o, mode; std::string pat; match_string_term(n, *t, o, mode, pat);
  return dict_entry_matches(e, mode, pat);
}
template <class Pred>
static std::vector<uint32_t> dict_lut(const Column& c, Pred&& holds) {
  std::vector<uint32_t> lut((size_t)(c.dict_n + 31) / 32, 0u);
  for (int32_t k = 0; k < c.dict_n; k++) if (holds(c.dict_host[(size_t)k])) lut[(size_t)k >> 5] |= 1u << (k & 31);
  return lut;
}
// ismissing(col) / !ismissing(col) over a nullable fixed-width column: its missing bitmap is the mask
static bool match_missing(dfdb_table* t, const Node& n, MissStep& out) {
  const Node* m = &n; bool neg = false;
  if (m->op == DFIR_NOT && m->a) { m = m->a.get(); neg = true; }
  if (m->op != DFIR_ISMISSING || !m->a || m->a->op != DFIR_COL) return false;
  const Column& col = need_resident(t, m->a->col);
  if (!dt_nullable(col.dtype) || dt_base(col.dtype) == DFDB_STRING || !col.missing.p) return false;
  out = MissStep{col.missing.as<uint64_t>(), neg};
  return true;
}
// a second comparison of a column the batch already compares folds into that term as an interval: `65 > x > 34` (test/selection.jl:53) reads x once
// instead of twice.  The transforms (rem / col * k + d) must agree too; the compressed-only scan takes untransformed terms only.
static bool fold_interval(ScanTerm& into, const ScanTerm& tm) {
  if (into.op2 >= 0 || into.dtype != tm.dtype || into.pre != tm.pre || (tm.pre != 0 && (into.pre_d != tm.pre_d || into.pre_magic != tm.pre_magic))) return false;
  into.op2 = tm.op; into.cbits2 = tm.cbits;
  return true;
}

// The launch that produces the query's final mask can do more with its LAST term (k_scan_terms EXTRA):
//   sum / min / max (dfdb_query_hint_aggregate): the hinted column is a term of the last batch of the last stage -> per-tile partials
//   capture (dfdb_query_hint_materialize): the last batch of the LAST stage is that launch, whatever ran before it in this stage (generic conjuncts, string
//   and dictionary scans, missing masks, disjunctions all come first and only hand it a mask to AND with) or in earlier stages.  Every projected plain 8-byte
//   column among its terms — up to two — is kept by the scan instead of gathered afterwards (round 4; round 1-3 captured one column of a single-stage
//   query whose only conjuncts were simple terms).
// The chosen term goes last in its batch (and the second captured one before it).
static void plan_rider(const dfdb_query* q, PredPlan& plan, bool last_stage) {
  if (plan.term_batches.empty()) return;
  const dfdb_ctx* ctx = q->t->ctx;
  TermBatch& lb = plan.term_batches.back();
  ScanTerms& ts = lb.terms;
  auto plain8 = [&](int k) { const int dt = ts.t[k].dtype; return !ts.t[k].pre && (dt == DFDB_I64 || dt == DFDB_U64 || dt == DFDB_F64); };   // (a rem term compares rem(x, m): not the value to add up or keep)
  int special = -1, special2 = -1;
  if ((q->hint_agg_op == DFDB_AGG_SUM || q->hint_agg_op == DFDB_AGG_MIN || q->hint_agg_op == DFDB_AGG_MAX) && last_stage && q->hint_agg_proj >= 0 &&
      (size_t)q->hint_agg_proj < q->proj.size()) {
    const Node& pe = *q->proj[(size_t)q->hint_agg_proj].expr;
    if (pe.op == DFIR_COL && !dt_nullable(pe.dtype))
      for (int k = 0; k < ts.n && special < 0; k++)
        if (plain8(k) && lb.ords[k] == pe.col) { special = k; plan.extra = q->hint_agg_op == DFDB_AGG_SUM ? EX_SUM : (q->hint_agg_op == DFDB_AGG_MIN ? EX_MIN : EX_MAX); }
  }
  if (plan.extra == EX_NONE && q->hint_materialize && last_stage && ctx_option(ctx, "scan_capture", 2) > 0) {
    const int maxcap = (int)std::min<int64_t>(2, ctx_option(ctx, "scan_capture", 2));
    for (int k = 0; k < ts.n && (special < 0 || (special2 < 0 && maxcap >= 2)); k++) {
      if (!plain8(k)) continue;
      if (special >= 0 && lb.ords[k] == lb.ords[special]) continue;     // (two terms of one column that did not fold)
      for (const ProjCol& p : q->proj) {
        bool wanted = p.expr->op == DFIR_COL && p.expr->col == lb.ords[k] && !dt_nullable(p.expr->dtype);
        if (!wanted && p.expr->op != DFIR_COL && dt_width(p.expr->dtype) == 8 && !dt_nullable(p.expr->dtype)) {
          // a computed column that is a transform of this one column (`x * 2`, `a % 7`, `a * 3 + 1`): it is made from the captured values too
          ScanTerm tf; const Node* tcol = nullptr;
          wanted = match_column_transform(p.expr.get(), tf, tcol) && tf.pre != 0 && tcol->col == lb.ords[k] && !dt_nullable(tcol->dtype);
        }
        if (wanted) { if (special < 0) { special = k; plan.extra = EX_CAPTURE; } else { special2 = k; plan.extra = EX_CAPTURE2; } break; }
      }
    }
  }
  if (plan.extra == EX_NONE) return;
  auto move_to = [&](int from, int to) { std::swap(ts.t[from], ts.t[to]); std::swap(lb.ords[from], lb.ords[to]); };
  move_to(special, ts.n - 1);
  if (plan.extra == EX_CAPTURE2) {
    if (special2 == ts.n - 1) special2 = special;                       // (it was sitting in the last place and has just been swapped away)
    move_to(special2, ts.n - 2);
  }
}

// classifies every conjunct, builds the look-up tables, decides the rider and the String capture.  No launch: the need_resident calls may queue the
// transient whole-column decode of a compressed-only column, all of them before the stage's first predicate launch.  (The String columns of string
// matches and pairs are checked here too, so "column ... is not resident" for one of them is raised before anything of the stage has been launched.)
static PredPlan plan_predicate(dfdb_query* q, const Node& pred, bool first_stage, bool last_stage) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx;
  PredPlan plan;
  std::vector<const Node*> conj, generic; flatten_and(pred, conj);
  // `s1 OP s2` over two String columns (and coalesce(s1 OP s2, false) over nullable ones): k_str_pair / k_dict_pair; ctx option "str_pair_kernel" = 0 leaves
  // it to the interpreter's H_STRCMP2, which is the definition
  const bool pair_kernel = ctx_option(ctx, "str_pair_kernel", 1) != 0;
  TermBatch cur{}; cur.terms.n = 0; cur.terms.combine_or = 0;
  for (const Node* c : conj) {
    ScanTerm tm; int ord, dord = -1; StrStep ss; PairStep ps{}; ScanTerms ob; MissStep ms;
    const Node* const inner = coalesce_false_arg(*c);      // coalesce(X, false): X, for the string routes that answer exactly that over nullable columns
    if (match_missing(t, *c, ms)) { plan.miss.push_back(ms); continue; }
    if ((c->op == DFIR_OR || c->op == DFIR_NOT || c->op == DFIR_XOR) && dict_only(t, *c, dord) && dord >= 0) {
      const Column& dc = t->cols[(size_t)dord];
      plan.dict_luts.push_back(DictLutStep{dord, dict_lut(dc, [&](const std::string& e) { return dict_eval(t, *c, e); })});
      continue;
    }
    if ((c->op == DFIR_OR || c->op == DFIR_IN_SET) && match_or(t, *c, ob)) { plan.or_batches.push_back(ob); continue; }
    const bool simple = match_simple_term(*c, *t, tm, ord);      // (once: a failed match leaves `tm` half-written)
    if (simple && comp_scannable(t, tm, ord)) {
      // a compressed-only column: the decoder evaluates the term (a second comparison of the same column folds into an interval there too)
      bool folded = false;
      for (CompStep& ct : plan.comp_terms) if (ct.ord == ord && fold_interval(ct.tm, tm)) { folded = true; break; }
      if (!folded) plan.comp_terms.push_back(CompStep{tm, ord});
    } else if (simple) {
      tm.col = need_resident(t, ord).data.p;
      bool folded = false;
      for (int k = 0; k < cur.terms.n && !folded; k++) folded = cur.ords[k] == ord && fold_interval(cur.terms.t[k], tm);
      if (folded) continue;
      if (cur.terms.n == kMaxTerms) { plan.term_batches.push_back(cur); cur.terms.n = 0; }
      cur.ords[cur.terms.n] = ord; cur.terms.t[cur.terms.n++] = tm;
    } else if (match_string_term(*c, *t, ss.ord, ss.mode, ss.pat) || (inner && match_string_term(*inner, *t, ss.ord, ss.mode, ss.pat, true))) {
      // (coalesce(s == "x", false) over a Union{String,Missing} column — the docs' real data set: index.md:264-272 — is K5's own answer, not the interpreter's)
      const Column& col = need_resident(t, ss.ord);
      if (col.dict_n > 0) ss.lut = dict_lut(col, [&](const std::string& e) { return dict_entry_matches(e, ss.mode, ss.pat); });
      plan.strs.push_back(std::move(ss));
    } else if (pair_kernel && (match_string_pair_term(*c, ps.a, ps.b, ps.op) || (inner && match_string_pair_term(*inner, ps.a, ps.b, ps.op, true)))) {
      (void)need_resident(t, ps.a); (void)need_resident(t, ps.b);
      plan.pairs.push_back(ps);
    } else generic.push_back(c);
  }
  if (cur.terms.n) plan.term_batches.push_back(cur);
  // Julia's fused `&` is not short-circuit (BlockBroadcasting(&, (old, elem)), selection.jl:44-47), so every generic conjunct is evaluated — and may raise
  // DivideError / InexactError — on every row that REACHED this stage, not only on the rows an earlier conjunct kept: one program, and the first step
  if (generic.size() == 1) plan.interp = generic[0];
  else if (!generic.empty()) {
    plan.interp_owned = generic[0]->clone();
    for (size_t i = 1; i < generic.size(); i++) plan.interp_owned = make_and(std::move(plan.interp_owned), generic[i]->clone());
    plan.interp = plan.interp_owned.get();
  }
  plan_rider(q, plan, last_stage);
  // String capture (see dfdb_query.hint_materialize): only when this stage is the whole query and exactly one step, a flat string match whose column is
  // itself projected — that ONE launch then produces the query's final mask, keeps the selected rows' sizes and bytes, and K6 never reads the column again.
  // (Every other step would run after it or hand it a mask, and narrow what it kept: the capture would hold rows the query drops — tests/test_gpu_fuzz.py.)
  if (q->hint_materialize && first_stage && q->stages.size() == 1 && plan.steps() == 1 && plan.strs.size() == 1) {
    const StrStep& st = plan.strs[0];
    const Column& col = t->cols[(size_t)st.ord];
    if (st.mode != 0 && !dt_nullable(col.dtype) && col.dict_n == 0 && st.pat.size() <= 64)
      for (const ProjCol& p : q->proj) if (p.expr->op == DFIR_COL && p.expr->col == st.ord) { plan.str_capture = true; break; }
  }
  return plan;
}

// "<family>.indexed" / ".recording" / ".plain": which form of an LZ4 decode launch the column's sequence-start index selected (column_lz4_index)
static void note_lz4_mode(dfdb_ctx* ctx, const char* family, int mode) {
  if (ctx->profiling) prof_note(ctx, (std::string(family) + (mode == 2 ? ".indexed" : mode == 1 ? ".recording" : ".plain")).c_str());
}

static void run_str_step(dfdb_query* q, const StrStep& st, bool have, bool do_cap) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const int64_t nrows = t->nrows;
  const Column& col = t->cols[(size_t)st.ord];
  // `col == "const"` is an AND-ed conjunct of this stage, and later stages only remove rows: every row the query finally selects holds exactly
  // `const` in this column, so its projection needs neither the column nor a capture (materialize_col: launch_fill_const_strings)
  if (st.mode == 0 && !dt_nullable(col.dtype)) { q->left.const_str_col = st.ord; q->left.const_str = st.pat; }
  // K9: the column has a dictionary — the term was decided once per distinct string on the host, the rows are a bit-table lookup of their codes
  if (col.dict_n > 0) { run_dict_scan(q, col, st.lut, have); return; }
  const std::string& pat = st.pat;
  DevBuf& pb = q->tmp_a; pb.ensure(pat.size() + 64);
  if (pat.size() > 16) { HIP_CHECK(hipMemcpyAsync(pb.p, pat.data(), pat.size(), hipMemcpyHostToDevice, s)); stream_wait(ctx); }   // (bytes past 16 are compared against the device copy)
  StrCapture capture{nullptr, nullptr, nullptr};
  if (do_cap) {
    const int64_t nt = ceil_div(nrows, kTileRows);
    q->cap_str_sizes.ensure((size_t)nt * kTileRows * 4 + 256);
    q->cap_str_bytes.ensure((size_t)col.nbytes + 256);
    q->cap_str_tb.ensure((size_t)(nt + 8) * 4);
    capture = StrCapture{q->cap_str_sizes.as<int32_t>(), q->cap_str_bytes.as<uint8_t>(), q->cap_str_tb.as<uint32_t>()};
  }
  LaunchTimer lt(ctx, "str_match");
  if (ctx->profiling) {                 // which form launch_str_match takes, for the tests that must meet every one (tests/test_gpu_str_match.py)
    const StrMatchForm form = str_match_form((int32_t)pat.size(), col.max_tile_bytes);
    prof_note(ctx, form == STR_MATCH_STAGED ? "str_match.staged" : form == STR_MATCH_DIRECT ? "str_match.direct" : "str_match.long");
  }
  launch_str_match(s, str_side(col), StrPattern{(const uint8_t*)pat.data(), pb.as<uint8_t>(), (int32_t)pat.size()}, st.mode, q->bitmap.as<uint64_t>(),
                   q->tile_counts.as<uint32_t>(), nrows, have, do_cap ? &capture : nullptr, col.max_tile_bytes);
  if (do_cap) q->left.cap_str_col = st.ord;
}
// (after the generic conjuncts like every other string scan: those see every row that reached the stage; a pair launch pins no constant and captures nothing)
static void run_pair_step(dfdb_query* q, const PairStep& pt, bool have) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx;
  const Column &ca = t->cols[(size_t)pt.a], &cb = t->cols[(size_t)pt.b];
  if (ca.dict_n > 0 && cb.dict_n > 0) { run_dict_pair(q, ca, cb, pt.op, have); return; }      // (a dictionary column is never nullable)
  LaunchTimer lt(ctx, "str_pair");
  launch_str_pair(ctx->stream, str_side(ca), str_side(cb), pt.op, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), t->nrows, have);
}
// a compressed-only column: one K7 launch per term — every block decoded into the waves' history rings, the comparison applied to the bytes as they leave
// the LDS ring, bitmap + tile counts the only output.  From the second mask on the words are AND-ed in and a block without a survivor
// is not decoded at all (blocksiterator.jl:111-113 at block granularity).
static void run_comp_step(dfdb_query* q, const CompStep& ct, bool have) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx;
  Column& fc = t->cols[(size_t)ct.ord];
  LzScan sc{q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), ct.tm.cbits, ct.tm.dtype, ct.tm.op};
  sc.op2 = ct.tm.op2; sc.cbits2 = ct.tm.cbits2; sc.and_existing = have ? 1 : 0;
  int waves = 0; uint8_t* scratch = ctx_hist_scratch(ctx, &waves);
  const int imode = column_lz4_index(ctx, fc, true);
  LaunchTimer lt(ctx, "lz4_decode_scan_hist");
  note_lz4_mode(ctx, "lz4_decode_scan_hist", imode);
  launch_lz4_decode_hist(ctx->stream, fc.comp.as<uint8_t>(), scratch, waves, fc.comp_blocks.as<Lz4Block>(), (int32_t)fc.comp_nblocks, fc.comp_status.as<int32_t>(), &sc,
                         fc.comp_index.as<uint32_t>(), imode);
  std::vector<int>& seen = q->left.comp_scanned;
  if (std::find(seen.begin(), seen.end(), ct.ord) == seen.end()) seen.push_back(ct.ord);
}

// the launch that writes a fresh mask over the whole column: run it against the bitmap allocation this column pairs best with (place_mask)
static void place_first_batch(dfdb_query* q, PredPlan& plan) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const ScanTerms tb0 = plan.term_batches[0].terms;
  const int ord0 = plan.term_batches[0].ords[0];
  const bool nt = true;                 // nontemporal column loads (the A/B knob "scan_nt" went in round 6: plain loads were never faster)
  const int wt0 = scan_store_flags(ctx);
  const void* const col_before = t->cols[(size_t)ord0].data.p;
  place_mask(q, ord0, [&](uint64_t* bm, int64_t rows, const void* colp) {
    ScanTerms tbx = tb0;                                          // the calibration may be trying another allocation of the first term's column
    for (int k = 0; k < tbx.n; k++) if (tbx.t[k].col == col_before) tbx.t[k].col = colp;
    if (tbx.n == 1 && tbx.t[0].op2 < 0 && tbx.t[0].pre == 0) launch_scan_cmp(s, tbx.t[0], bm, q->tile_counts.as<uint32_t>(), rows, false, nt, nullptr, wt0);
    else launch_scan_terms(s, tbx, bm, q->tile_counts.as<uint32_t>(), rows, false, EX_NONE, nullptr, (int)ctx_option(ctx, "scan_pair", 1));
  });
  const void* const col_after = t->cols[(size_t)ord0].data.p;
  if (col_after == col_before) return;
  auto follow = [&](ScanTerms& ts) { for (int k = 0; k < ts.n; k++) if (ts.t[k].col == col_before) ts.t[k].col = col_after; };
  for (TermBatch& b : plan.term_batches) follow(b.terms);           // the column was re-placed: every term of this stage that reads it follows
  for (ScanTerms& ob : plan.or_batches) follow(ob);
}

// decode -> scan fusion: a fresh-mask scan of ONE simple term over an 8-byte column that holds its LZ4 blocks in HBM
// (ctx option keep_compressed at load time) decodes the blocks and evaluates the term in the same pass (K7 SCAN): what the reference's loop
// body does per block (read_block! then apply the selection, blocksiterator.jl:98-121).  ctx option "decode_on_scan" = 1 asks for it;
// the decoded column is (re)written on the way, so everything after this launch sees an ordinary resident column.
// Returns whether the launch it queued also answered the term (false: only a decode, or nothing — the ordinary scan follows).
static bool run_decode_on_scan(dfdb_query* q, const ScanTerm& tm, int ord) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  Column& fc = t->cols[(size_t)ord];
  const int fdt = tm.dtype;
  if (!(fc.comp_nblocks > 0 && !dt_nullable(fc.dtype) && (fdt == DFDB_I64 || fdt == DFDB_U64 || fdt == DFDB_F64) && t->block_size % kTileRows == 0)) return false;
  q->left.decoded_col = ord;                           // query_count looks at the blocks' statuses where it waits for the count anyway
  // few blocks (every one resident in the two-wave pipeline at once): the pipeline, then the ordinary scan of the decoded column, is the shorter way —
  // a block's latency is what a small launch pays, and the fused form is one wave per block (1 526 blocks: 328 GB/s + a 0.13-ms scan against ~210 GB/s fused)
  const int pipe = (int)ctx_option(ctx, "lz4_pipeline", -1);
  if (pipe == 1 || (pipe < 0 && fc.comp_nblocks <= 2048)) {
    const int dmode = column_lz4_index(ctx, fc, lz4_decode_takes_index((int32_t)fc.comp_nblocks, pipe));
    LaunchTimer lt(ctx, "lz4_decode");
    note_lz4_mode(ctx, "lz4_decode", dmode);
    launch_lz4_decode(s, fc.comp.as<uint8_t>(), fc.data.as<uint8_t>(), fc.comp_blocks.as<Lz4Block>(), (int32_t)fc.comp_nblocks, fc.comp_status.as<int32_t>(), pipe,
                      fc.comp_index.as<uint32_t>(), dmode);
    return false;
  }
  const int imode = column_lz4_index(ctx, fc, true);
  LaunchTimer lt(ctx, "lz4_decode_scan");
  note_lz4_mode(ctx, "lz4_decode_scan", imode);
  launch_lz4_decode_scan(s, fc.comp.as<uint8_t>(), fc.data.as<uint8_t>(), fc.comp_blocks.as<Lz4Block>(), (int32_t)fc.comp_nblocks, fc.comp_status.as<int32_t>(),
                         LzScan{q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), tm.cbits, fdt, tm.op}, fc.comp_index.as<uint32_t>(), imode);
  return true;
}
// one batch of AND-ed simple terms; ex: the rider (the plan's, on its last batch).  fresh_first: this launch writes the first mask of the query's first stage
static void run_term_batch(dfdb_query* q, const TermBatch& b, int ex, bool have, bool fresh_first) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const ScanTerms& tb = b.terms;
  const bool one_plain = tb.n == 1 && tb.t[0].op2 < 0 && tb.t[0].pre == 0;
  if (one_plain && ex == EX_NONE && fresh_first && ctx_option(ctx, "decode_on_scan", 0) != 0 && run_decode_on_scan(q, tb.t[0], b.ords[0])) return;
  if (one_plain && ex == EX_NONE && run_image_scan(q, b.ords[0], tb.t[0], have)) return;      // answered from the column's scan copies (scan_image.cpp)
  if (one_plain && (ex == EX_NONE || (ex == EX_CAPTURE && !have))) {      // (k_scan_cmp captures over a fresh mask only)
    LaunchTimer lt(ctx, "scan_cmp");
    prof_note(ctx, ctx_option(ctx, "scan_wt_store", 1) ? "scan_cmp.wt_store" : "scan_cmp.plain_store");
    launch_scan_cmp(s, tb.t[0], q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), t->nrows, have,
                    true, ex == EX_CAPTURE ? q->cap_buf.p : nullptr, scan_store_flags(ctx));
    return;
  }
  LaunchTimer lt(ctx, "scan_terms");
  const int pair = (int)ctx_option(ctx, "scan_pair", 1);
  if (pair && scan_pair_applies(tb, have)) prof_note(ctx, "scan_terms.pair");
  launch_scan_terms(s, tb, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), t->nrows, have, ex, ex_captures(ex) ? q->cap_buf.p : ex_reduces(ex) ? q->agg_partials.p : nullptr, pair,
                    ex == EX_CAPTURE2 ? q->cap_buf2.p : nullptr);
}

static void run_plan(dfdb_query* q, PredPlan& plan, bool first_stage) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const int64_t nrows = t->nrows;
  bool have = !first_stage;   // does the bitmap already hold a mask to AND with?  Every step ANDs into it from the second on: advanced here and nowhere else
  auto step = [&](auto&& launch) { launch(have); have = true; };
  if (plan.interp) step([&](bool h) { run_interp_predicate(q, *plan.interp, h); });
  for (const DictLutStep& dl : plan.dict_luts) step([&](bool h) { run_dict_scan(q, t->cols[(size_t)dl.ord], dl.lut, h); });
  for (const StrStep& st : plan.strs) step([&](bool h) { run_str_step(q, st, h, plan.str_capture); });
  for (const PairStep& pt : plan.pairs) step([&](bool h) { run_pair_step(q, pt, h); });
  for (const MissStep& mt : plan.miss) step([&](bool h) {
    LaunchTimer lt(ctx, "missing_mask");
    launch_missing_mask(s, mt.bits, mt.negate, h, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), nrows);
  });
  for (const ScanTerms& ob : plan.or_batches) step([&](bool h) {
    LaunchTimer lt(ctx, "scan_terms");
    launch_scan_terms(s, ob, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), nrows, h, EX_NONE, nullptr);
  });
  for (const CompStep& ct : plan.comp_terms) step([&](bool h) { run_comp_step(q, ct, h); });
  if (plan.term_batches.empty()) return;
  if (plan.extra == EX_CAPTURE2) q->cap_buf2.ensure((size_t)round_up(nrows, kTileRows) * 8 + 256);
  if (ex_captures(plan.extra)) q->cap_buf.ensure((size_t)round_up(nrows, kTileRows) * 8 + 256);
  else if (plan.extra != EX_NONE) q->agg_partials.ensure((size_t)(ceil_div(nrows, kTileRows) + 8) * 8);
  const bool fresh = !have && first_stage;
  if (fresh) place_first_batch(q, plan);
  for (size_t bi = 0; bi < plan.term_batches.size(); bi++)
    step([&](bool h) { run_term_batch(q, plan.term_batches[bi], bi + 1 == plan.term_batches.size() ? plan.extra : (int)EX_NONE, h, fresh && bi == 0); });
  const TermBatch& lb = plan.term_batches.back();
  const int last = lb.terms.n - 1;
  if (ex_captures(plan.extra)) q->left.cap_col = lb.ords[last];
  if (plan.extra == EX_CAPTURE2) q->left.cap_col2 = lb.ords[last - 1];
  if (ex_reduces(plan.extra)) { q->left.agg_col = lb.ords[last]; q->left.agg_dtype = lb.terms.t[last].dtype; q->left.agg_op = q->hint_agg_op; }
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
  q->count = -1; q->prefix_valid = false; q->executed_stages = -1;
  q->left = dfdb_query::Left{};
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
    if (st.kind == ST_PRED) {
      PredPlan plan = plan_predicate(q, *st.pred, i == 0, i + 1 == (int)q->stages.size());
      run_plan(q, plan, i == 0);
      q->prefix_valid = false;
    }
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

void ensure_executed(dfdb_query* q) {
  if (!reflects_all_stages(q) || q->bitmap_rows != q->t->nrows) query_execute(q, -1);
}

int64_t query_count(dfdb_query* q, int nstages);
// ensure_executed for a consumer that hands results to the HOST (or builds on them: unique, groupreduce, a new column): an execution that decoded a column's
// resident LZ4 blocks on its way (decode_on_scan) is only as good as that decode, and the blocks' statuses are read — and a failed decode repeated once
// without the index — where query_count waits for the count (only dfdb_count did so).  Consumers that stay asynchronous on the device
// (dfdb_select_indices / _bitmap into device memory without a count, the group layer's device aggregates) are covered by the caller's next dfdb_count or
// dfdb_table_decode_status, as include/dfdb.h says.
void ensure_executed_checked(dfdb_query* q) {
  ensure_executed(q);
  if (q->left.decoded_col >= 0 || !q->left.comp_scanned.empty()) (void)query_count(q, -1);
}

static int64_t read_total(dfdb_query* q) {
  dfdb_ctx* ctx = q->t->ctx;
  HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, q->prefix.as<uint64_t>() + ceil_div(q->t->nrows, kTileRows), 8, hipMemcpyDeviceToHost, ctx->stream));
  stream_wait(ctx);
  return ctx->pinned_scalar[0];
}
// the columns whose LZ4 blocks the last execution decoded on its way: inside its scan (compressed-only: several terms may have, each column's statuses
// are its last launch's) / ahead of it (decode_on_scan)
static std::vector<int> comp_scanned_cols(const dfdb_query* q) { return q->left.comp_scanned; }
static std::vector<int> decode_on_scan_cols(const dfdb_query* q) { return q->left.decoded_col >= 0 ? std::vector<int>{q->left.decoded_col} : std::vector<int>{}; }
// An execution that decoded a column's resident LZ4 blocks on its way has results only as good as that decode: a block K7 gave up on (a damaged copy, or
// err 9 — a sequence-start index that is not this stream's) leaves stale mask words, tile counts and column bytes behind.  A bad block drops the index
// (table_decode_status); ONE more execution decodes by parsing and records a new one; bad again -> the blocks themselves are damaged.  `cols` is read
// again after that execution (it starts q->left afresh).  Returns whether it executed again: the total is to be read again.
static bool redo_bad_decode(dfdb_query* q, int nstages, std::vector<int> (*cols)(const dfdb_query*)) {
  bool again = false;
  for (int col : cols(q)) again = table_decode_status(q->t, col) > 0 || again;
  if (!again) return false;
  query_execute(q, nstages);
  for (int col : cols(q)) {
    const int64_t bad = table_decode_status(q->t, col);
    if (bad > 0) { q->executed_stages = -1; fail(DFDB_ERR_FORMAT, "column %s: %lld of its resident LZ4 blocks do not decode", q->t->cols[(size_t)col].name.c_str(), (long long)bad); }
  }
  return true;
}

int64_t query_count(dfdb_query* q, int nstages) {
  if (nstages < 0) { ensure_executed(q); if (q->count >= 0) return q->count; }
  else query_execute(q, nstages);
  int64_t n = read_total(q);
  // the statuses are read here, where the host waits for the count anyway
  if (redo_bad_decode(q, nstages < 0 ? -1 : nstages, comp_scanned_cols)) n = read_total(q);
  if (redo_bad_decode(q, nstages < 0 ? -1 : nstages, decode_on_scan_cols)) n = read_total(q);
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

}  // namespace dfdb
