// ooc.cpp — out-of-core execution behind the ordinary query entry points (ooc.hpp).
//
// What the reference's consumers do block by block over a BlocksIterator, done chunk by chunk over the block stream of stream.cpp:
//   nrow(v)              view.jl:192-206 + blocksiterator.jl:46-66,123-145  (BlockRowsIterator: the selection's columns only)      -> ooc_count
//   materialize(v)       materialization.jl:27-40 (count pre-pass for sizehint!, then append! per block)                          -> ooc_materialize
//   sum / minimum / ...  Base.iterate(::DFColumn) column.jl:102-126                                                               -> ooc_aggregate
//   unique(col)          Base.unique over the same iteration (docs/src/index.md:171-182,479-487)                                  -> ooc_unique
//   groupreduce          aggregate.jl:1-36 (completed as dfdb_query_groupreduce completes it)                                     -> ooc_groupreduce
// HBM holds the stream's chunks (ctx option "stream_slots" x "ooc_chunk_blocks" blocks per required column), never the table.
#include "ooc.hpp"
#include <algorithm>
#include <cmath>

namespace dfdb {

// ------------------------------------------------------------------ folding and the by-key merge (shared with group.cpp)
template <class T> static T fold_t(T a, T b, int op) { return op == DFDB_AGG_MIN ? std::min(a, b) : (op == DFDB_AGG_MAX ? std::max(a, b) : (T)(a + b)); }
uint64_t fold_bits(uint64_t a, uint64_t b, int dt, int op) {
  if (op == DFDB_AGG_SUM && dt != DFDB_F64) return a + b;
  if (dt == DFDB_F64) {
    double x, y; memcpy(&x, &a, 8); memcpy(&y, &b, 8);
    const double r = op == DFDB_AGG_SUM ? x + y : minmax_f64(x, y, op == DFDB_AGG_MIN);
    uint64_t o; memcpy(&o, &r, 8); return o;
  }
  if (dt == DFDB_U64) return fold_t<uint64_t>(a, b, op);
  return (uint64_t)fold_t<int64_t>((int64_t)a, (int64_t)b, op);
}

// isequal as a byte string, appended to k: the missing flag, then the value's bytes with every NaN folded onto one (isequal(NaN, -NaN); -0.0 and 0.0 stay apart)
static void merge_key(std::string& k, int32_t kdt, const GroupKeys& p, int64_t j, int64_t& byte_off) {
  const bool miss = !p.key_missing.empty() && p.key_missing[(size_t)j];
  const size_t flag = k.size();
  k.push_back(miss ? '\1' : '\0');
  if (dt_base(kdt) == DFDB_STRING) {
    int32_t sz; memcpy(&sz, p.key_data.data() + (size_t)j * 4, 4);
    if (sz < 0) { k[flag] = '\1'; return; }
    k.append((const char*)p.key_bytes.data() + byte_off, (size_t)sz); byte_off += sz;
    return;
  }
  if (miss) return;                                      // (the bytes under a missing flag are garbage: quirk Q11)
  const int w = dt_width(kdt);
  const uint8_t* v = p.key_data.data() + (size_t)j * w;
  if (dt_base(kdt) == DFDB_F64) { double d; memcpy(&d, v, 8); if (std::isnan(d)) { k.append("NaN"); return; } }
  if (dt_base(kdt) == DFDB_F32) { float f; memcpy(&f, v, 4); if (std::isnan(f)) { k.append("NaN"); return; } }
  k.append((const char*)v, (size_t)w);
}

void GroupMerger::add(GroupMerged& m, const GroupPart& p) {
  const size_t nk = m.key_dtypes.size(), nv = m.ops.size();
  if (p.keys.size() != nk || p.vals.size() != nv) fail(DFDB_ERR_DEVICE, "group merge: a part of %zu key columns and %zu reducers among parts of %zu and %zu", p.keys.size(), p.vals.size(), nk, nv);
  const bool rows = !p.first_rows.empty();
  std::vector<int64_t> boff(nk, 0), b0(nk);
  std::vector<size_t> at(nk);                              // where key i's image starts in k
  std::string k;
  for (int64_t j = 0; j < p.ng; j++) {                     // part order = table order: a tuple keeps the place of its first appearance
    k.clear();
    for (size_t i = 0; i < nk; i++) {
      b0[i] = boff[i];
      k.append(4, '\0'); at[i] = k.size();
      merge_key(k, m.key_dtypes[i], p.keys[i], j, boff[i]);
      const uint32_t len = (uint32_t)(k.size() - at[i]);
      memcpy(&k[at[i] - 4], &len, 4);
    }
    const auto ins = slot.try_emplace(k, m.ng);
    if (ins.second) {
      m.ng++;
      for (size_t i = 0; i < nk; i++) {
        GroupKeys& km = m.keys[i]; const GroupKeys& kp = p.keys[i];
        const bool is_str = dt_base(m.key_dtypes[i]) == DFDB_STRING;
        const int w = is_str ? 4 : dt_width(m.key_dtypes[i]);
        km.key_data.insert(km.key_data.end(), kp.key_data.begin() + j * w, kp.key_data.begin() + (j + 1) * w);
        km.key_missing.push_back(k[at[i]] == '\1' ? 1 : 0);
        if (is_str) km.key_bytes.insert(km.key_bytes.end(), kp.key_bytes.begin() + b0[i], kp.key_bytes.begin() + boff[i]);
      }
      m.counts.push_back(p.counts[(size_t)j]);
      for (size_t r = 0; r < nv; r++) m.vals[r].push_back(p.vals[r][(size_t)j]);
      if (rows) m.first_rows.push_back(p.first_rows[(size_t)j]);
      continue;
    }
    const size_t s = (size_t)ins.first->second;
    m.counts[s] += p.counts[(size_t)j];
    for (size_t r = 0; r < nv; r++) {
      const uint64_t a = m.vals[r][s], b = p.vals[r][(size_t)j];
      if (m.ops[r] == DFDB_AGG_COUNT) m.vals[r][s] = a + b;
      else m.vals[r][s] = fold_bits(a, b, kind_dtype(m.kinds[r]), m.ops[r]);   // wrapping Int sums, Float64 sums of the parts' sums, NaN-propagating min / max
    }
  }
}

void fetch_group_part(dfdb_query* q, const int32_t* key_cols, int32_t nkeys, const int32_t* val_cols, const int32_t* stats, int32_t nvals, bool with_rows, GroupPart& part) {
  int64_t ng = 0;
  std::vector<int64_t> kb((size_t)nkeys, 0);
  query_groupreduce_n(q, key_cols, nkeys, val_cols, stats, nvals, &ng, kb.data());   // (one key with at most one reducer: query_groupreduce itself)
  part.ng = ng; part.keys.resize((size_t)nkeys);
  std::vector<dfdb_outcol> outs((size_t)nkeys);
  for (int k = 0; k < nkeys; k++) {
    const int32_t kdt = q->proj[(size_t)key_cols[k]].expr->dtype;
    const bool is_str = dt_base(kdt) == DFDB_STRING;
    GroupKeys& kp = part.keys[(size_t)k];
    kp.key_data.resize((size_t)ng * (size_t)(is_str ? 4 : dt_width(kdt)));
    if (dt_nullable(kdt) && !is_str) kp.key_missing.assign((size_t)ng, 0);
    kp.key_bytes.resize((size_t)kb[(size_t)k]);
    dfdb_outcol& oc = outs[(size_t)k];
    oc = dfdb_outcol{}; oc.memkind = DFDB_MEM_HOST; oc.data = kp.key_data.data(); oc.bytes = kp.key_bytes.data(); oc.bytes_cap = kb[(size_t)k];
    oc.missing = kp.key_missing.empty() ? nullptr : kp.key_missing.data();
  }
  part.counts.assign((size_t)ng, 0);
  if (with_rows) {                                         // between groupreduce and its fetch q's selection IS the first occurrences (dfdb.h)
    part.first_rows.assign((size_t)ng, 0);
    if (ng > 0) { int64_t got = 0; query_select_indices(q, part.first_rows.data(), ng, DFDB_MEM_HOST, &got); if (got != ng) fail(DFDB_ERR_DEVICE, "groupreduce: %lld first rows for %lld groups", (long long)got, (long long)ng); }
  }
  std::vector<int64_t> vi((size_t)ng * (size_t)nvals); std::vector<double> vf((size_t)ng * (size_t)nvals);
  query_groupreduce_n_fetch(q, outs.data(), part.counts.data(), vi.data(), vf.data());   // (puts the full selection back)
  part.vals.assign((size_t)nvals, std::vector<uint64_t>((size_t)ng));
  for (int r = 0; r < nvals; r++) {
    const size_t r0 = (size_t)r * (size_t)ng;
    if (stats[r] != DFDB_AGG_COUNT && q->gr_kinds_n[(size_t)r] == 2) { if (ng > 0) memcpy(part.vals[(size_t)r].data(), vf.data() + r0, (size_t)ng * 8); }
    else for (int64_t j = 0; j < ng; j++) part.vals[(size_t)r][(size_t)j] = (uint64_t)vi[r0 + (size_t)j];
  }
}

void merged_fetch(const GroupMerged& m, dfdb_outcol* keys, int64_t* counts, int64_t* vals_i, double* vals_f, bool single_key) {
  const size_t ng = (size_t)m.ng;
  if (keys) for (size_t i = 0; i < m.key_dtypes.size(); i++) {
    dfdb_outcol* o = &keys[i];
    const GroupKeys& km = m.keys[i];
    if (o->memkind != DFDB_MEM_HOST) fail(DFDB_ERR_ARGUMENT, "merged keys are written to host buffers");
    o->dtype = m.key_dtypes[i]; o->count = m.ng; o->nbytes = (int64_t)km.key_bytes.size();
    if (ng == 0) continue;
    if (!o->data) fail(DFDB_ERR_ARGUMENT, "the key column has no data buffer");
    memcpy(o->data, km.key_data.data(), km.key_data.size());
    if (o->missing) memcpy(o->missing, km.key_missing.data(), ng);
    if (dt_base(m.key_dtypes[i]) == DFDB_STRING && !km.key_bytes.empty()) {
      if ((int64_t)km.key_bytes.size() > o->bytes_cap || !o->bytes) fail(DFDB_ERR_ARGUMENT, "the key column needs %zu string bytes, capacity is %lld", km.key_bytes.size(), (long long)o->bytes_cap);
      memcpy(o->bytes, km.key_bytes.data(), km.key_bytes.size());
    }
  }
  if (counts && ng > 0) memcpy(counts, m.counts.data(), ng * 8);
  for (size_t r = 0; r < m.vals.size(); r++)
    group_values_out(m.vals[r].data(), m.ng, m.ops[r] == DFDB_AGG_COUNT ? 0 : m.kinds[r], vals_i ? vals_i + r * ng : nullptr, vals_f ? vals_f + r * ng : nullptr);
  if (single_key && m.vals.empty()) { if (vals_i) std::fill_n(vals_i, ng, 0); if (vals_f) std::fill_n(vals_f, ng, 0.0); }
}

// ------------------------------------------------------------------ which queries stream
static void view_columns(const dfdb_query* q, std::vector<int>& sel, std::vector<int>& all) {
  for (const Stage& st : q->stages) if (st.kind == ST_PRED) required_columns(*st.pred, sel);
  all = sel;
  for (const ProjCol& p : q->proj) required_columns(*p.expr, all);
}
bool query_out_of_core(const dfdb_query* q) {
  const dfdb_table* t = q->t;
  if (!t || t->path.empty() || q->stream_owned) return false;
  std::vector<int> sel, all;
  view_columns(q, sel, all);
  if (all.empty()) {
    // no column is needed (range stages only and an empty projection or one of constants): the row count comes from the first column, like the stream's
    if (t->cols.empty()) return false;
    return !t->cols[0].resident && t->nrows < 0;
  }
  for (int o : all) if (!t->cols[(size_t)o].resident) return true;
  return false;
}

static OocState& state(dfdb_query* q) {
  if (!q->ooc) q->ooc = std::make_shared<OocState>();
  if (q->ooc->str_bytes.size() != q->proj.size()) q->ooc->str_bytes.assign(q->proj.size(), -1);
  return *q->ooc;
}
void ooc_reset(dfdb_query* q) { if (q->ooc) { const dfdb_sizestats keep = q->ooc->read; q->ooc = std::make_shared<OocState>(); q->ooc->read = keep; } }

// the caller's view re-stated with another projection (and, for a narrowed query, another selection): what a pass streams
struct TempQuery {
  dfdb_query q;
  TempQuery(const dfdb_query* src, bool with_stages, int nstages = -1) {
    q.t = src->t;
    if (with_stages)
      for (const Stage& st : src->stages) {
        if (nstages >= 0 && (int)q.stages.size() >= nstages) break;
        Stage c; c.kind = st.kind; c.start = st.start; c.step = st.step; c.stop = st.stop; c.n = st.n; c.idx = st.idx; c.stage_base = st.stage_base;
        if (st.pred) c.pred = st.pred->clone();
        q.stages.push_back(std::move(c));
      }
  }
  void project(const ProjCol& p) { q.proj.push_back(ProjCol{p.name, p.expr->clone()}); }
  void project_column(const dfdb_table* t, int o) {
    auto n = std::make_unique<Node>(); n->op = DFIR_COL; n->col = o; n->dtype = t->cols[(size_t)o].dtype;
    q.proj.push_back(ProjCol{t->cols[(size_t)o].name, std::move(n)});
  }
};

// one pass of the block stream over `tq`; fn(chunk) for every chunk in table order
struct StreamPass {
  dfdb_stream* s = nullptr;
  dfdb_query* owner;
  StreamPass(dfdb_query* owner_, dfdb_query* tq) : owner(owner_) {
    const int64_t cb = ctx_option(tq->t->ctx, "ooc_chunk_blocks", 512);
    stream_open(tq, cb > 0 ? cb : 512, &s);
  }
  dfdb_query* next() { int64_t rows = 0, first = 0; return stream_next(s, &rows, &first); }
  ~StreamPass() {
    if (!s) return;
    try {
      dfdb_sizestats st{0, 0, 0};
      stream_read_stats(s, -1, &st);
      OocState& o = state(owner);
      o.read.rows += st.rows; o.read.compressed += st.compressed; o.read.uncompressed += st.uncompressed;
    } catch (...) {}
    try { stream_close(s); } catch (...) {}
  }
  StreamPass(const StreamPass&) = delete;
  StreamPass& operator=(const StreamPass&) = delete;
};

// a query narrowed by dfdb_query_unique: its selection is the first occurrences' table rows
static void narrowed_view(dfdb_query* q, TempQuery& tq) {
  OocState& o = state(q);
  Stage st; st.kind = ST_INDICES; st.idx = o.merged.first_rows;
  query_add_stage(&tq.q, std::move(st));
}

// ------------------------------------------------------------------ count
// The row counter reads the selection's columns only — or, when the queue holds no predicate, the FIRST projection column (blocksiterator.jl:46-66) —
// never a projection-only column.  With dfdb_query_hint_materialize on, the pass also sizes the projected String columns (their sizes are read for the
// blocks that kept a row: late materialization), so that count + materialize stay two passes like the reference's (materialization.jl:29-37).
int64_t ooc_count(dfdb_query* q) {
  OocState& o = state(q);
  if (o.narrowed) return o.merged.ng;
  if (o.count >= 0) return o.count;
  const dfdb_table* t = q->t;
  std::vector<int> sel, all;
  view_columns(q, sel, all);
  TempQuery tq(q, true);
  std::vector<int> sized;                             // projection columns of q sized in this pass -> their position in tq's projection
  std::vector<int> pos;
  // (no column needed at all: a projection of constants iterates nothing — `isempty(it.streams)`, blocksiterator.jl:101 —, an EMPTY projection counts the
  // selection off the first column's block sizes: both are the stream's own rules, so the projection goes over as it is)
  if (all.empty()) { for (const ProjCol& p : q->proj) tq.project(p); }
  else tq.project_column(t, sel.empty() ? all[0] : sel[0]);
  if (q->hint_materialize && !all.empty())
    for (size_t p = 0; p < q->proj.size(); p++) {
      const Node& e = *q->proj[p].expr;
      if (dt_base(e.dtype) != DFDB_STRING || e.op != DFIR_COL) continue;
      bool dup = false;
      for (size_t k = 0; k < tq.q.proj.size(); k++) if (tq.q.proj[k].expr->op == DFIR_COL && tq.q.proj[k].expr->col == e.col) { sized.push_back((int)p); pos.push_back((int)k); dup = true; break; }
      if (dup) continue;
      sized.push_back((int)p); pos.push_back((int)tq.q.proj.size());
      tq.project(q->proj[p]);
    }
  int64_t total = 0;
  std::vector<int64_t> sb(sized.size(), 0);
  {
    StreamPass pass(q, &tq.q);
    while (dfdb_query* c = pass.next()) {
      const int64_t n = query_count(c, -1);
      total += n;
      if (n > 0) for (size_t k = 0; k < sized.size(); k++) sb[k] += query_string_bytes(c, pos[k]);
    }
  }
  for (size_t k = 0; k < sized.size(); k++) o.str_bytes[(size_t)sized[k]] = sb[k];
  return o.count = total;
}

void ooc_select_indices(dfdb_query* q, int64_t* out, int64_t cap, int32_t memkind, int64_t* n) {
  OocState& o = state(q);
  if (o.narrowed) {
    const int64_t m = std::min<int64_t>(cap, o.merged.ng);
    if (n) *n = o.merged.ng;
    if (m <= 0) return;
    if (memkind == DFDB_MEM_DEVICE) { HIP_CHECK(hipMemcpyAsync(out, o.merged.first_rows.data(), (size_t)m * 8, hipMemcpyHostToDevice, q->t->ctx->stream)); HIP_CHECK(hipStreamSynchronize(q->t->ctx->stream)); }
    else memcpy(out, o.merged.first_rows.data(), (size_t)m * 8);
    return;
  }
  const dfdb_table* t = q->t;
  std::vector<int> sel, all;
  view_columns(q, sel, all);
  TempQuery tq(q, true);
  if (all.empty()) { for (const ProjCol& p : q->proj) tq.project(p); }
  else tq.project_column(t, sel.empty() ? all[0] : sel[0]);
  int64_t total = 0;
  {
    StreamPass pass(q, &tq.q);
    while (dfdb_query* c = pass.next()) {
      const int64_t k = query_count(c, -1);
      if (k > 0 && total < cap) {
        int64_t got = 0;
        query_select_indices(c, out + total, cap - total, memkind, memkind == DFDB_MEM_DEVICE ? nullptr : &got);
        if (memkind == DFDB_MEM_DEVICE) HIP_CHECK(hipStreamSynchronize(c->t->ctx->stream));   // (the chunk's buffers are reused by the next one)
      }
      total += k;
    }
  }
  o.count = total;
  if (n) *n = total;
}

// ------------------------------------------------------------------ materialize
static int64_t width_of(const Node& e) { return dt_base(e.dtype) == DFDB_STRING ? 4 : dt_width(e.dtype); }

// every chunk's rows appended to the caller's buffers at the running offsets (append!(res, bl), materialization.jl:33-37)
static void stream_materialize(dfdb_query* q, dfdb_query* tq, dfdb_outcol* outs, int32_t ncols, int64_t row_cap) {
  std::vector<int64_t> boff((size_t)ncols, 0);
  int64_t rows = 0;
  int32_t dts_set = 0;
  {
    StreamPass pass(q, tq);
    std::vector<dfdb_outcol> so((size_t)ncols);
    while (dfdb_query* c = pass.next()) {
      const int64_t n = query_count(c, -1);
      if (n == 0) continue;
      if (row_cap >= 0 && rows + n > row_cap) fail(DFDB_ERR_BOUNDS, "BoundsError: the view holds more rows than were counted (%lld): the table's files changed between dfdb_count and dfdb_materialize", (long long)row_cap);
      for (int32_t p = 0; p < ncols; p++) {
        dfdb_outcol x = outs[p];
        const Node& e = *tq->proj[(size_t)p].expr;
        if (x.data) x.data = (char*)x.data + rows * width_of(e);
        if (x.bytes) { x.bytes += boff[(size_t)p]; x.bytes_cap = outs[p].bytes_cap - boff[(size_t)p]; }
        if (x.missing) x.missing += rows;
        so[(size_t)p] = x;
      }
      query_materialize(c, so.data(), ncols);
      HIP_CHECK(hipStreamSynchronize(c->t->ctx->stream));   // device outputs are queued on the CHUNK's stream: done before the chunk goes
      for (int32_t p = 0; p < ncols; p++) { boff[(size_t)p] += so[(size_t)p].nbytes; outs[p].dtype = so[(size_t)p].dtype; }
      dts_set = 1;
      rows += n;
    }
  }
  for (int32_t p = 0; p < ncols; p++) {
    if (!dts_set) outs[p].dtype = tq->proj[(size_t)p].expr->dtype;
    outs[p].count = rows; outs[p].nbytes = boff[(size_t)p];
  }
  OocState& o = state(q);
  if (!o.narrowed) { o.count = rows; for (int32_t p = 0; p < ncols; p++) if (dt_base(tq->proj[(size_t)p].expr->dtype) == DFDB_STRING) o.str_bytes[(size_t)p] = boff[(size_t)p]; }
}

int64_t ooc_string_bytes(dfdb_query* q, int32_t i) {
  if (i < 0 || (size_t)i >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", i);
  const Node& e = *q->proj[(size_t)i].expr;
  if (dt_base(e.dtype) != DFDB_STRING) return 0;
  if (e.op != DFIR_COL && !is_string_coalesce(e)) fail(DFDB_ERR_UNSUPPORTED, "computed String columns are outside the IR");
  OocState& o = state(q);
  if (o.narrowed && e.op == DFIR_COL && o.merged_col == e.col) return (int64_t)o.merged.keys[0].key_bytes.size();
  if (!o.narrowed && o.str_bytes[(size_t)i] >= 0) return o.str_bytes[(size_t)i];
  // a sizing pass of its own: the selection with this one column as its projection
  TempQuery tq(q, !o.narrowed);
  if (o.narrowed) narrowed_view(q, tq);
  tq.project(q->proj[(size_t)i]);
  int64_t total = 0, rows = 0;
  {
    StreamPass pass(q, &tq.q);
    while (dfdb_query* c = pass.next()) { const int64_t n = query_count(c, -1); rows += n; if (n > 0) total += query_string_bytes(c, 0); }
  }
  if (!o.narrowed) { o.str_bytes[(size_t)i] = total; o.count = rows; }
  return total;
}

void ooc_materialize(dfdb_query* q, dfdb_outcol* outs, int32_t ncols) {
  if (ncols != (int32_t)q->proj.size()) fail(DFDB_ERR_ARGUMENT, "ArgumentError: view has %zu columns, %d outputs given", q->proj.size(), ncols);
  OocState& o = state(q);
  if (o.narrowed) {
    // unique(col): the key column comes out of the merged first occurrences; any other column is read at those rows
    bool only_key = true;
    for (const ProjCol& p : q->proj) only_key = only_key && p.expr->op == DFIR_COL && p.expr->col == o.merged_col;
    if (only_key) {
      for (int32_t p = 0; p < ncols; p++) {
        if (outs[p].memkind != DFDB_MEM_HOST) { only_key = false; break; }
      }
    }
    if (only_key) { for (int32_t p = 0; p < ncols; p++) merged_fetch(o.merged, &outs[p], nullptr, nullptr, nullptr, true); return; }
    TempQuery tq(q, false);
    narrowed_view(q, tq);
    for (const ProjCol& p : q->proj) tq.project(p);
    stream_materialize(q, &tq.q, outs, ncols, o.merged.ng);
    return;
  }
  if (ncols == 0) return;
  TempQuery tq(q, true);
  for (const ProjCol& p : q->proj) tq.project(p);
  stream_materialize(q, &tq.q, outs, ncols, o.count);
}

void ooc_materialize_column(dfdb_query* q, int32_t p, dfdb_outcol* o) {
  if (p < 0 || (size_t)p >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", p);
  OocState& st = state(q);
  TempQuery tq(q, !st.narrowed);
  if (st.narrowed) narrowed_view(q, tq);
  tq.project(q->proj[(size_t)p]);
  const int64_t cap = st.narrowed ? st.merged.ng : st.count;
  // (stream_materialize keeps what it learns under the projection index of the query it streams: a one-column pass must not overwrite column 0's string bytes)
  const std::vector<int64_t> keep = st.str_bytes;
  stream_materialize(q, &tq.q, o, 1, cap);
  state(q).str_bytes = keep;
}

// ------------------------------------------------------------------ aggregates
void ooc_aggregate(dfdb_query* q, int32_t op, int32_t i, int64_t* out_i, double* out_f) {
  if (op == DFDB_AGG_COUNT) { const int64_t n = ooc_count(q); if (out_i) *out_i = n; if (out_f) *out_f = (double)n; return; }
  if (i < 0 || (size_t)i >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", i);
  const Node& e = *q->proj[(size_t)i].expr;
  if (!dt_isnum(e.dtype) || dt_nullable(e.dtype)) fail(DFDB_ERR_UNSUPPORTED, "aggregate over %s is not supported", dt_name(e.dtype).c_str());
  OocState& o = state(q);
  TempQuery tq(q, !o.narrowed);
  if (o.narrowed) narrowed_view(q, tq);
  tq.project(q->proj[(size_t)i]);
  const int adt = agg_dtype(e.dtype);                     // the accumulator query_aggregate_device reduces in
  uint64_t acc = 0; bool have = false; int64_t rows = 0;
  {
    StreamPass pass(q, &tq.q);
    while (dfdb_query* c = pass.next()) {
      const int64_t n = query_count(c, -1);
      if (n == 0) continue;                              // (minimum / maximum of an empty chunk would raise)
      rows += n;
      int64_t vi = 0; double vf = 0;
      query_aggregate(c, op, 0, &vi, &vf);
      uint64_t bits; if (adt == DFDB_F64) memcpy(&bits, &vf, 8); else bits = (uint64_t)vi;
      acc = have ? fold_bits(acc, bits, adt, op) : bits;  // chunk order = block order = the reference's left-to-right order at chunk granularity
      have = true;
    }
  }
  if (!o.narrowed) o.count = rows;
  if (!have) {
    if (op != DFDB_AGG_SUM) fail(DFDB_ERR_ARGUMENT, "ArgumentError: reducing over an empty collection is not allowed");
    acc = 0;                                             // (0 and 0.0 share a bit pattern)
  }
  group_values_out(&acc, 1, value_kind(adt), out_i, out_f);
}

// ------------------------------------------------------------------ unique / groupreduce
// the resident dfdb_query_groupreduce_n per chunk, the chunks merged by key tuple in chunk order (= first appearance) -> state(q).merged.
// by_prefix: groupreduce_check's — the streamed dfdb_query_unique and dfdb_query_groupreduce name both in the refusal of a computed key column
static void stream_groupreduce(dfdb_query* q, const int32_t* key_cols, int32_t nkeys, const int32_t* val_cols, const int32_t* stats, int32_t nvals, bool with_rows,
                               const char* by_prefix) {
  GroupMerged m;
  m.kinds = groupreduce_check(q, key_cols, nkeys, val_cols, stats, nvals, by_prefix);
  m.ops.assign(stats, stats + nvals);
  for (int k = 0; k < nkeys; k++) m.key_dtypes.push_back(q->proj[(size_t)key_cols[k]].expr->dtype);
  m.keys.resize((size_t)nkeys); m.vals.resize((size_t)nvals);
  OocState& o = state(q);
  if (o.narrowed) fail(DFDB_ERR_ARGUMENT, "ArgumentError: the query's selection is narrowed by dfdb_query_unique: dfdb_query_reset it first");
  // the chunk query projects the keys, then the reducers' columns (a count reads none)
  TempQuery tq(q, true);
  std::vector<int32_t> kidx((size_t)nkeys), vidx((size_t)nvals, -1);
  for (int k = 0; k < nkeys; k++) { kidx[(size_t)k] = (int32_t)tq.q.proj.size(); tq.project(q->proj[(size_t)key_cols[k]]); }
  for (int r = 0; r < nvals; r++) if (stats[r] != DFDB_AGG_COUNT) { vidx[(size_t)r] = (int32_t)tq.q.proj.size(); tq.project(q->proj[(size_t)val_cols[r]]); }
  GroupMerger mg;
  int64_t rows = 0;
  {
    StreamPass pass(q, &tq.q);
    while (dfdb_query* c = pass.next()) {
      const int64_t n = query_count(c, -1);
      if (n == 0) continue;
      rows += n;
      GroupPart part;
      fetch_group_part(c, kidx.data(), nkeys, vidx.data(), stats, nvals, with_rows, part);
      mg.add(m, part);
    }
  }
  m.valid = true;
  o.count = rows;
  o.merged = std::move(m);
  o.merged_col = q->proj[(size_t)key_cols[0]].expr->col;
  o.pending = OocState::NONE;
}

void ooc_unique(dfdb_query* q, int32_t p) {
  stream_groupreduce(q, &p, 1, nullptr, nullptr, 0, true, "unique / ");
  state(q).narrowed = true;
}

void ooc_groupreduce(dfdb_query* q, int32_t key_p, int32_t val_p, int32_t op, int64_t* ngroups, int64_t* key_bytes) {
  stream_groupreduce(q, &key_p, 1, &val_p, &op, op == DFDB_AGG_COUNT ? 0 : 1, false, "unique / ");   // (a count has no value array)
  OocState& o = state(q);
  o.pending = OocState::GROUPREDUCE;
  if (ngroups) *ngroups = o.merged.ng;
  if (key_bytes) *key_bytes = (int64_t)o.merged.keys[0].key_bytes.size();
}

void ooc_groupreduce_n(dfdb_query* q, const int32_t* key_cols, int32_t nkeys, const int32_t* val_cols, const int32_t* stats, int32_t nvals, int64_t* ngroups,
                       int64_t* key_bytes) {
  stream_groupreduce(q, key_cols, nkeys, val_cols, stats, nvals, false, "");
  OocState& o = state(q);
  o.pending = OocState::GROUPREDUCE_N;
  if (ngroups) *ngroups = o.merged.ng;
  if (key_bytes) for (int k = 0; k < nkeys; k++) key_bytes[k] = (int64_t)o.merged.keys[(size_t)k].key_bytes.size();
}

void ooc_groupreduce_fetch(dfdb_query* q, OocState::Pending which, dfdb_outcol* keys, int64_t* counts, int64_t* vals_i, double* vals_f) {
  OocState& o = state(q);
  const bool single = which == OocState::GROUPREDUCE;
  if (o.pending != which || !o.merged.valid)
    fail(DFDB_ERR_ARGUMENT, "ArgumentError: dfdb_query_groupreduce%s has not been called (or the query was executed, reset or changed since)", single ? "" : "_n");
  merged_fetch(o.merged, keys, counts, vals_i, vals_f, single);
  o.merged = GroupMerged{}; o.pending = OocState::NONE; o.merged_col = -1;
}

// ------------------------------------------------------------------ what a multi-GPU group asks of a shard that is not resident (group.cpp)
// survivors of stages [0, nstages) over the shard's block window: the operand of the all-gather between a predicate stage and a range stage after it
int64_t ooc_count_prefix(dfdb_query* q, int nstages) {
  const dfdb_table* t = q->t;
  TempQuery tq(q, true, nstages);
  std::vector<int> sel, all;
  view_columns(&tq.q, sel, all);
  if (!sel.empty()) tq.project_column(t, sel[0]);
  else { std::vector<int> s2, a2; view_columns(q, s2, a2); if (!a2.empty()) tq.project_column(t, a2[0]); }
  int64_t total = 0;
  StreamPass pass(q, &tq.q);
  while (dfdb_query* c = pass.next()) total += query_count(c, -1);
  return total;
}
// {value bits, selected rows} of sum / min / max over projection column i, the identity of `op` when nothing is selected (what query_aggregate_device
// leaves in red_result); returns the accumulator dtype
int ooc_aggregate_bits(dfdb_query* q, int32_t op, int32_t i, uint64_t out[2]) {
  if (i < 0 || (size_t)i >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", i);
  const Node& e = *q->proj[(size_t)i].expr;
  if (!dt_isnum(e.dtype) || dt_nullable(e.dtype)) fail(DFDB_ERR_UNSUPPORTED, "aggregate over %s is not supported", dt_name(e.dtype).c_str());
  const int adt = agg_dtype(e.dtype);
  const int64_t n = ooc_count(q);
  if (n == 0) {
    out[0] = reduce_identity_bits(value_kind(adt), op == DFDB_AGG_MIN, op == DFDB_AGG_MAX); out[1] = 0;
    return adt;
  }
  int64_t vi = 0; double vf = 0;
  ooc_aggregate(q, op, i, &vi, &vf);
  if (adt == DFDB_F64) memcpy(&out[0], &vf, 8); else out[0] = (uint64_t)vi;
  out[1] = (uint64_t)n;
  return adt;
}
// the shard's groups as ONE part (its chunks merged in chunk order), for the merge across the ranks
int ooc_group_part(dfdb_query* q, int32_t key_p, int32_t val_p, int32_t op, GroupPart& part) {
  stream_groupreduce(q, &key_p, 1, &val_p, &op, op == DFDB_AGG_COUNT ? 0 : 1, false, "unique / ");
  OocState& o = state(q);
  const int kind = o.merged.kinds.empty() ? 0 : o.merged.kinds[0];
  part = std::move(static_cast<GroupPart&>(o.merged));
  o.merged = GroupMerged{}; o.merged_col = -1;
  return kind;
}

// ------------------------------------------------------------------ dfdb_query_prepare
// Only the columns the view needs are opened (view.jl:183-190, blocksiterator.jl:20-33).  They become resident when they fit: decoded if the decoded arrays
// (plus the load's staging of the compressed bytes) fit the budget, compressed-only (LZ4 blocks in HBM, K7 decodes inside the scan) if those fit and every
// missing column is a plain fixed-width one, and otherwise they stay on disk and the entry points stream.
int32_t query_prepare(dfdb_query* q) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx;
  if (t->path.empty()) return 0;
  std::vector<int> sel, all;
  view_columns(q, sel, all);
  if (all.empty() && !t->cols.empty() && t->nrows < 0) all.push_back(0);
  std::vector<int32_t> need;
  for (int o : all) if (!t->cols[(size_t)o].resident) need.push_back(o);
  if (need.empty()) return 0;
  HIP_CHECK(hipSetDevice(ctx->device));
  // two bounds: what the TABLE may hold (ctx option "hbm_budget_mb"; 0 = no bound of its own) and what the device has free right now (the load's staging of
  // one column file and, for the compressed-only form, the context's history rings come out of that too)
  HbmRoom room;
  HIP_CHECK(table_hbm_room(t, &room));
  int64_t dec = 0, comp = 0, comp_max = 0; bool plain = true;
  for (int32_t o : need) {
    dfdb_sizestats st{0, 0, 0};
    table_column_stats(t, o, &st);
    dec += st.uncompressed; comp += st.compressed; comp_max = std::max(comp_max, st.compressed);
    const Column& c = t->cols[(size_t)o];
    plain = plain && dt_base(c.dtype) != DFDB_STRING && !dt_nullable(c.dtype);
  }
  auto unload = [&] { for (int32_t o : need) { Column& c = t->cols[(size_t)o]; if (!c.resident) { drop_scan_image(ctx, c); c.data.release(); c.bytes.release(); c.missing.release(); c.tile_off.release(); c.comp.release(); c.comp_blocks.release(); c.comp_status.release(); c.comp_index.release(); c.comp_nblocks = 0; c.comp_only = false; } } };
  const int64_t kc_old = ctx_option(ctx, "keep_compressed", 0);
  struct Restore { dfdb_ctx* c; int64_t v; ~Restore() { c->options["keep_compressed"] = v; } } restore{ctx, kc_old};
  if (dec <= room.budget && dec + comp_max + (64 << 20) <= room.free_now) {           // decoded arrays (+ the staging of one column file at a time)
    if (kc_old == 2) ctx->options["keep_compressed"] = 0;
    try { table_load(t, need.data(), (int32_t)need.size(), 0, -1, nullptr); return 1; }
    catch (const Error& e) { if (e.code != DFDB_ERR_NOMEM) throw; (void)hipGetLastError(); unload(); }
  }
  const int64_t held = comp + comp / 8;                                      // the blocks + their sequence-start index
  int waves = 0; const bool rings = ctx->hist.p != nullptr; (void)waves;
  if (plain && held <= room.budget && held + comp_max + (rings ? 0 : (int64_t)lz4_hist_scratch_bytes(lz4_hist_default_waves(ctx->prop.multiProcessorCount))) + (64 << 20) <= room.free_now) {
    ctx->options["keep_compressed"] = 2;
    try { table_load(t, need.data(), (int32_t)need.size(), 0, -1, nullptr); return 2; }
    catch (const Error& e) { if (e.code != DFDB_ERR_NOMEM) throw; (void)hipGetLastError(); unload(); }
  }
  return 3;
}

}  // namespace dfdb
