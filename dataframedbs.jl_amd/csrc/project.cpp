// project.cpp — the projection side of a DFView on the device: what is made of the rows a query selected.  Materialize (fixed-width gathers, the String
// output arena and its offsets, captured columns, computed columns), the survivors' arena of a compressed-only column, add_column! from a view, aggregates.
//
// Replaces (paths in the reference tree): ProjectionExecutor.eval_on_range src/tables/projection.jl:128-154, materialize
// src/tables/materialization.jl:27-52, add_column!(table, name, lazy_col) src/tables/table.jl:96-124.
//
// The selection itself — stages, bitmap, prefix scan, count — is query.cpp's; everything here starts from an executed query (ensure_executed) and reads
// what that execution left behind in dfdb_query::left.
#include "engine.hpp"
#include "ooc.hpp"
#include "select_key.hpp"
#include <algorithm>

namespace dfdb {

// launchers living in k_interp.hip / k_parse.hip that take engine-level descriptions
void run_interp_project(dfdb_query* q, const Node& expr, void* dst, int64_t cap, uint8_t* missing_dst);
void run_str_convert(dfdb_query* q, const Node& expr, void* dst, int64_t cap);   // k_parse.hip


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

// ---------------------------------------------------------------- String output columns
static bool string_captured(const dfdb_query* q, const Column& col) {
  return q->left.cap_str_col >= 0 && &q->t->cols[(size_t)q->left.cap_str_col] == &col && reflects_all_stages(q);
}

// What a String projection column is made of: column `a` and what stands behind its missing rows — nothing (the column itself), or the constant or the column b
// of coalesce(a, b) (expr.hpp is_string_coalesce) — and which producer writes the selected rows:
//   STR_CONST_FILL  every selected row holds the constant of a conjunct `a == "const"` (query.cpp run_str_step): the constant, count times
//   STR_DICT        K9: the selected rows' dictionary codes, expanded
//   STR_CAPTURED    K5 kept the selected rows while it matched: one contiguous copy per tile
//   STR_GATHER      K6 reads the flat sizes and bytes through the bitmap, in the form of `fill`
// What the execution left behind for a plain projection of `a` — K5's capture, "every selected row holds the constant", the compacted dictionary codes —
// answers for a's own rows, not for the coalesced ones: a coalesce is always STR_GATHER
enum StrProducer { STR_CONST_FILL, STR_DICT, STR_CAPTURED, STR_GATHER };
struct StrSource { const Column* a; StrFillKind fill; const Column* b; const std::string* k; StrProducer by; };

static StrSource string_source(dfdb_query* q, const Node& e) {
  if (is_string_coalesce(e)) {
    const Column& a = need_resident(q->t, e.a->col);
    if (e.b->op == DFIR_COL) return StrSource{&a, STR_FILL_COL, &need_resident(q->t, e.b->col), nullptr, STR_GATHER};
    return StrSource{&a, STR_FILL_CONST, nullptr, &e.b->str, STR_GATHER};
  }
  if (e.op != DFIR_COL) fail(DFDB_ERR_UNSUPPORTED, "computed String columns are outside the IR");
  const Column& a = need_resident(q->t, e.col);
  const StrProducer by = q->left.const_str_col == e.col && reflects_all_stages(q) ? STR_CONST_FILL
                         : a.dict_n > 0 ? STR_DICT : string_captured(q, a) ? STR_CAPTURED : STR_GATHER;
  return StrSource{&a, STR_FILL_NONE, nullptr, nullptr, by};
}
static StrFill str_fill(const StrSource& src, const uint8_t* const_dev) {
  return StrFill{src.fill, src.b ? str_side(*src.b) : StrSide{nullptr, nullptr, nullptr}, const_dev, src.k ? (int32_t)src.k->size() : 0};
}

// a constant on the device (q->tmp_a), with room behind it for copy_string's 8-byte tail load; waits for the upload (`k` may be gone after the call)
static const uint8_t* upload_constant(dfdb_query* q, const std::string& k) {
  dfdb_ctx* ctx = q->t->ctx;
  DevBuf& kb = q->tmp_a; kb.ensure(k.size() + 64);
  if (!k.empty()) { HIP_CHECK(hipMemcpyAsync(kb.p, k.data(), k.size(), hipMemcpyHostToDevice, ctx->stream)); stream_wait(ctx); }
  return kb.as<uint8_t>();
}

// selected string bytes per 1024-row tile -> exclusive scan into tile_off_out (output arena offsets), the selected sizes -> dst_sizes (`cap` rows); returns
// the byte total.  (STR_CONST_FILL has its total without a launch; STR_CAPTURED leaves dst_sizes to the copy)
static int64_t string_out_offsets(dfdb_query* q, const StrSource& src, int32_t* dst_sizes, int64_t cap, DevBuf& tile_off_out) {
  if (src.by == STR_CONST_FILL) return cap * (int64_t)q->left.const_str.size();
  dfdb_ctx* ctx = q->t->ctx; hipStream_t s = ctx->stream;
  const Column& col = *src.a;
  const int64_t nct = ceil_div(q->t->nrows, kTileRows);
  DevBuf& tb = q->tmp_c; tb.ensure((size_t)(nct + 8) * 4);
  tile_off_out.ensure((size_t)(nct + 8) * 8);
  DevBuf& scratch = q->str_scratch; scratch.ensure(scan_counts_scratch_bytes(nct));
  // per-tile totals -> exclusive scan into tile_off_out; the grand total comes back through pinned_scalar[1] (waits)
  auto scan_total = [&](const uint32_t* totals, int64_t ntiles) -> int64_t {
    launch_scan_counts(s, totals, tile_off_out.as<uint64_t>(), ntiles, scratch.as<uint64_t>());
    HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar + 1, tile_off_out.as<uint64_t>() + ntiles, 8, hipMemcpyDeviceToHost, s));
    stream_wait(ctx);
    return ctx->pinned_scalar[1];
  };
  if (src.by == STR_DICT) {
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
    return scan_total(otb.as<uint32_t>(), not_);
  }
  if (src.by == STR_CAPTURED) return scan_total(q->cap_str_tb.as<uint32_t>(), nct);     // K5 kept the selected rows: their byte totals per tile are already there
  { LaunchTimer lt(ctx, src.fill == STR_FILL_NONE ? "str_gather_sizes" : "str_coalesce_sizes");
    launch_str_gather_sizes(s, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), str_side(col), str_fill(src, nullptr), dst_sizes, tb.as<uint32_t>(), q->t->nrows, cap); }
  return scan_total(tb.as<uint32_t>(), nct);
}

// the sizes staging buffer (q->str_sizes, reused across calls: hipFree would sync the device) for `cnt` rows
static int32_t* string_sizes_staging(dfdb_query* q, int64_t cnt) { q->str_sizes.ensure((size_t)std::max<int64_t>(cnt, 1) * 4); return q->str_sizes.as<int32_t>(); }

int64_t query_string_bytes(dfdb_query* q, int i) {
  ensure_executed_checked(q);
  if (i < 0 || (size_t)i >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", i);
  const Node& e = *q->proj[(size_t)i].expr;
  if (dt_base(e.dtype) != DFDB_STRING) return 0;
  const StrSource src = string_source(q, e);
  const int64_t cnt = query_count(q, -1);
  return string_out_offsets(q, src, string_sizes_staging(q, cnt), cnt, q->str_toff);
}

// Where the producers of a String output column write: the caller's own buffers (device output: stream-ordered, never waited on) or the query's staging
// buffers (host output: copied back and waited for by finish()).  The sizes are there from the start, the bytes once the total is known
struct StrOut {
  dfdb_query* q; dfdb_outcol& o; int64_t cnt; bool dev;
  int32_t* sizes; uint8_t* bytes = nullptr;
  StrOut(dfdb_query* q_, dfdb_outcol& o_, int64_t cnt_)
      : q(q_), o(o_), cnt(cnt_), dev(o_.memkind == DFDB_MEM_DEVICE), sizes(dev ? (int32_t*)o_.data : string_sizes_staging(q_, cnt_)) {}
  void reserve_bytes(int32_t p, int64_t total) {
    o.nbytes = total;
    if (total > o.bytes_cap) fail(DFDB_ERR_ARGUMENT, "output column %d needs %lld string bytes, capacity is %lld", p, (long long)total, (long long)o.bytes_cap);
    bytes = dev ? o.bytes : (q->str_bytes.ensure((size_t)total + 64), q->str_bytes.as<uint8_t>());
  }
  void finish() {
    if (dev) return;
    dfdb_ctx* ctx = q->t->ctx;
    HIP_CHECK(hipMemcpyAsync(o.data, sizes, (size_t)cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (o.nbytes > 0) HIP_CHECK(hipMemcpyAsync(o.bytes, bytes, (size_t)o.nbytes, hipMemcpyDeviceToHost, ctx->stream));
    stream_wait(ctx);
  }
};

// one String output column (FlatStringsVector gather, FlatStringsVectors.jl:136-157; coalesce over Strings: no row raises)
static void materialize_string(dfdb_query* q, const StrSource& src, int32_t p, dfdb_outcol& o, int64_t cnt) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const Column& col = *src.a;
  DevBuf& toff = q->str_toff;
  StrOut out(q, o, cnt);
  const int64_t total = string_out_offsets(q, src, out.sizes, cnt, toff);
  out.reserve_bytes(p, total);
  switch (src.by) {
    case STR_CONST_FILL: {
      const uint8_t* pat = upload_constant(q, q->left.const_str);
      LaunchTimer lt(ctx, "fill_const_strings");
      launch_fill_const_strings(s, out.sizes, out.bytes, cnt, pat, (int32_t)q->left.const_str.size());
    } break;
    case STR_DICT:                     // the compacted codes of string_out_offsets -> bytes out of the dictionary
      if (total > 0) {
        LaunchTimer lt(ctx, "dict_expand_bytes");
        launch_dict_expand_bytes(s, q->dict_sel.as<uint16_t>(), cnt, col.dict_len.as<int32_t>(), col.dict_off.as<uint32_t>(), col.dict_bytes.as<uint8_t>(), toff.as<uint64_t>(), out.bytes, total);
      }
      break;
    case STR_CAPTURED: {               // sizes and bytes: one contiguous copy per tile out of the match pass's capture
      LaunchTimer lt(ctx, "str_compact_captured");
      const StrCapture sc{q->cap_str_sizes.as<int32_t>(), q->cap_str_bytes.as<uint8_t>(), q->cap_str_tb.as<uint32_t>()};
      launch_str_compact_captured(s, sc, q->prefix.as<uint64_t>(), (const int64_t*)col.tile_off.p, toff.as<uint64_t>(), out.sizes, out.bytes, t->nrows, cnt, total);
    } break;
    case STR_GATHER:
      if (total > 0) {
        const StrFill fill = str_fill(src, src.fill == STR_FILL_CONST ? upload_constant(q, *src.k) : nullptr);
        LaunchTimer lt(ctx, src.fill == STR_FILL_NONE ? "str_gather_bytes" : "str_coalesce_bytes");
        launch_str_gather_bytes(s, q->bitmap.as<uint64_t>(), str_side(col), fill, toff.as<uint64_t>(), out.bytes, t->nrows, total);
      }
      break;
  }
  out.finish();
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
  if (dt_base(e.dtype) == DFDB_STRING) { materialize_string(q, string_source(q, e), p, o, cnt); return; }
  if (e.op == DFIR_COL) {   // ColProjExec: buffer .= data[name][range] (projection.jl:130-133)
    const void* gsrc = nullptr;
    if (t->cols[(size_t)e.col].comp_only && !dt_nullable(e.dtype)) {
      if (!t->cols[(size_t)e.col].resident) fail(DFDB_ERR_ARGUMENT, "column %s is not resident on the device (dfdb_table_load it first)", t->cols[(size_t)e.col].name.c_str());
      gsrc = gather_source(q, e.col);        // compressed-only: the blocks with survivors, decoded for this query (no whole-column decode)
    }
    const Column& col = gsrc ? t->cols[(size_t)e.col] : need_resident(t, e.col);
    if (!gsrc) gsrc = col.data.p;
    DevBuf stage; void* dst = o.data;
    if (!dev) { stage.ensure((size_t)cnt * w); dst = stage.p; }
    if ((q->left.cap_col == e.col || q->left.cap_col2 == e.col) && w == 8 && reflects_all_stages(q)) {   // the scan kept these values: contiguous copy per tile
      LaunchTimer lt(ctx, "compact_captured");
      launch_compact_captured(s, (q->left.cap_col == e.col ? q->cap_buf : q->cap_buf2).as<uint64_t>(), q->prefix.as<uint64_t>(), (uint64_t*)dst, t->nrows, cnt);
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
    DevBuf stage, mstage; void* dst = o.data;
    if (!dev) { stage.ensure((size_t)cnt * w); dst = stage.p; }
    uint8_t* mdst = nullptr;                               // Union{R,Missing} result: one flag byte per selected row
    if (dt_nullable(e.dtype) && o.missing) { mdst = o.missing; if (!dev) { mstage.ensure((size_t)cnt); mdst = mstage.as<uint8_t>(); } }
    // a transform of ONE plain column (rem / col * k + d / col / k: expr.cpp match_column_transform) rides on the gather of that column
    ScanTerm tf; const Node* tcol = nullptr;
    if (w == 8 && !dt_nullable(e.dtype) && match_column_transform(&e, tf, tcol) && tf.pre != 0 && !dt_nullable(tcol->dtype) && t->cols[(size_t)tcol->col].resident) {
      const Column& sc = t->cols[(size_t)tcol->col];
      if ((q->left.cap_col == tcol->col || q->left.cap_col2 == tcol->col) && dt_width(sc.dtype) == 8 && reflects_all_stages(q)) {
        LaunchTimer lt(ctx, "compact_captured");                  // the scan kept the column's selected values: the transform rides on the copy
        launch_compact_captured_transform(s, (q->left.cap_col == tcol->col ? q->cap_buf : q->cap_buf2).as<uint64_t>(), q->prefix.as<uint64_t>(), dt_base(sc.dtype), tf, (uint64_t*)dst, t->nrows, cnt);
      } else {
        LaunchTimer lt(ctx, "gather");
        launch_gather_transform(s, q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), gather_source(q, tcol->col), dt_base(sc.dtype), tf, dst, t->nrows, cnt);
      }
    } else if (e.op == DFIR_CAST && e.a->op == DFIR_COL && dt_base(e.a->dtype) == DFDB_STRING && ctx_option(ctx, "parse_kernel", 1) != 0)
      // exactly parse.(T, s) or datetime19.(s): the conversion kernel (k_parse.hip); "parse_kernel" = 0: the interpreter
      run_str_convert(q, e, dst, cnt);
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
  c.logical = e.op == DFIR_COL ? q->t->cols[(size_t)e.col].logical : e.logical;   // a projected Date / DateTime / Char column keeps its type; datetime19(s) is a DateTime
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
  if (op == q->left.agg_op && e.op == DFIR_COL && q->left.agg_col == e.col && reflects_all_stages(q)) {
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
    dt = agg_dtype(q->left.agg_dtype);
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
  return agg_dtype(dt);
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

// Most-significant-digit radix select (k_select.hip) of up to kSelectMaxRanks ranks among the selected, non-missing values of `col`: one histogram pass per 8
// key bits, the bins chosen here in between.  Every rank carries the key bits decided so far (its prefix) and its position inside the bin they name; ranks with
// one prefix are one group of the pass.  `choose` names the ranks (1-based, R.n <= max_ranks of them) once cnt = {not missing, missing, NaN} of the selected rows
// is known: at once when the caller gives cnt (count = false), else after the first pass, which counts them — until then every possible rank shares the
// empty prefix, one group.  R.n = 0 ends the select (a counting pass alone when max_ranks = 0).  Returns R.n; keys[i] is the select key of rank i.
int select_keys(dfdb_query* q, const Column& col, bool full, bool count, int max_ranks, int64_t cnt[3], const std::function<void(SelectRanks&)>& choose, uint64_t* keys) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  SelectRanks R{}; bool chosen = false;
  uint64_t prefix[kSelectMaxRanks] = {}; int64_t rel[kSelectMaxRanks] = {};     // per rank
  if (!count) { choose(R); chosen = true; for (int i = 0; i < R.n; i++) rel[i] = R.rank[i]; if (R.n == 0) return 0; }
  DevBuf& st = q->tmp_a; st.ensure((size_t)(kSelectMaxRanks * 256 + 8) * 8);       // histograms, then the three counts
  uint64_t* hist = st.as<uint64_t>(); uint64_t* dcnt = hist + kSelectMaxRanks * 256;
  std::vector<uint64_t> h((size_t)kSelectMaxRanks * 256 + 8);
  const int nbits = select_key_bits(dt_base(col.dtype), full);
  for (int shift = nbits - 8; shift >= 0; shift -= 8) {
    SelectPass P{}; P.shift = shift; P.first = shift == nbits - 8 && count;
    int grp[kSelectMaxRanks];
    const int pending = chosen ? R.n : max_ranks;
    for (int i = 0; i < pending; i++) {
      int g = 0;
      while (g < P.ngroups && P.prefix[g] != prefix[i]) g++;
      if (g == P.ngroups) P.prefix[P.ngroups++] = prefix[i];
      grp[i] = g;
    }
    const size_t used = P.first ? h.size() : (size_t)P.ngroups * 256;
    HIP_CHECK(hipMemsetAsync(hist, 0, used * 8, s));
    { LaunchTimer lt(ctx, "select_hist");
      launch_select_hist(s, q->bitmap.as<uint64_t>(), q->tile_counts.as<uint32_t>(), col_ref(col), full, t->nrows, P, hist, dcnt); }
    HIP_CHECK(hipMemcpyAsync(h.data(), hist, used * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));            // (`h` is pageable host memory)
    if (P.first) for (int k = 0; k < 3; k++) cnt[k] = (int64_t)h[(size_t)kSelectMaxRanks * 256 + k];
    if (!chosen) { choose(R); chosen = true; for (int i = 0; i < R.n; i++) rel[i] = R.rank[i]; if (R.n == 0) return 0; }
    for (int i = 0; i < R.n; i++) {                // the bin that holds rank i of its group; the rank becomes relative to it
      const uint64_t* hg = h.data() + (size_t)grp[i] * 256;
      int b = 0;
      while (b < 256 && (uint64_t)rel[i] > hg[b]) { rel[i] -= (int64_t)hg[b]; b++; }
      if (b == 256) fail(DFDB_ERR_DEVICE, "radix select: the histogram of key bits %d.. holds fewer rows than the rank", shift);
      prefix[i] = (prefix[i] << 8) | (uint64_t)b;
    }
  }
  for (int i = 0; i < R.n; i++) keys[i] = prefix[i];
  return R.n;
}

// the k-th smallest values of projection column p over the selected rows (dfdb_order_statistics: Statistics.median / quantile over
// Base.iterate(::DFColumn), column.jl:102-126) by radix select (select_keys above)
void query_order_statistics(dfdb_query* q, int32_t p, const int64_t* ranks, int32_t nranks, int64_t* out_i, double* out_f, int64_t* counts) {
  if (nranks < 0 || nranks > kSelectMaxRanks) fail(DFDB_ERR_ARGUMENT, "ArgumentError: order statistics take 0 to %d ranks per call, %d given", kSelectMaxRanks, nranks);
  if (p < 0 || (size_t)p >= q->proj.size()) fail(DFDB_ERR_BOUNDS, "BoundsError: projection column %d", p);
  const Node& e = *q->proj[(size_t)p].expr;
  if (dt_base(e.dtype) == DFDB_STRING) fail(DFDB_ERR_ARGUMENT, "ArgumentError: order statistics of a String column are not defined");
  if (e.op != DFIR_COL) fail(DFDB_ERR_UNSUPPORTED, "order statistics of a computed column: materialise it as a column first (dfdb_table_add_from_query)");
  if (!dt_isnum(e.dtype)) fail(DFDB_ERR_UNSUPPORTED, "order statistics over %s are not supported", dt_name(e.dtype).c_str());
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx;
  // the column must be resident decoded: the block-streamed form and the one over the resident LZ4 blocks are follow-ups
  if (query_out_of_core(q)) fail(DFDB_ERR_UNSUPPORTED, "order statistics over a view that is out of core (its columns are not resident) are not supported: dfdb_table_load the columns first");
  if (t->cols[(size_t)e.col].comp_only)
    fail(DFDB_ERR_UNSUPPORTED, "order statistics over the compressed-only column %s (keep_compressed = 2) are not supported: dfdb_table_decode_resident it first", t->cols[(size_t)e.col].name.c_str());
  ensure_executed_checked(q);
  const Column& col = need_resident(t, e.col);
  const int dt = dt_base(e.dtype), kind = value_kind(dt);
  const bool nullable = dt_nullable(e.dtype), full = ctx_option(ctx, "select_full_image", 0) != 0;
  int64_t cnt[3] = {0, 0, 0};
  uint64_t keys[kSelectMaxRanks] = {};
  if (nranks == 0 && !nullable && kind != kAccFloat) cnt[0] = query_count(q, -1);   // nothing can be missing or NaN: the selection's own count
  else select_keys(q, col, full, true, nranks, cnt, [&](SelectRanks& R) {
    for (int i = 0; i < nranks; i++) {
      if (ranks[i] < 1 || ranks[i] > cnt[0]) fail(DFDB_ERR_BOUNDS, "BoundsError: rank %lld of %lld ordered values", (long long)ranks[i], (long long)cnt[0]);
      R.rank[i] = ranks[i];
    }
    R.n = nranks;
  }, keys);
  for (int i = 0; i < nranks; i++) {
    const uint64_t bits = select_key_value(dt, full, keys[i]);
    if (kind == kAccFloat) { if (out_f) out_f[i] = bits_f64(bits); }
    else { if (out_i) out_i[i] = (int64_t)bits; if (out_f) out_f[i] = kind == kAccUnsigned ? (double)bits : (double)(int64_t)bits; }
  }
  if (counts) for (int k = 0; k < 3; k++) counts[k] = cnt[k];
}

}  // namespace dfdb
