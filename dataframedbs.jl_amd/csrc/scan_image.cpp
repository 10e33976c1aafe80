// scan_image.cpp — the scan copies of a column (engine.hpp ScanCopies): built, read by lone `col OP const` scans, dropped.  The rule is scan_route.hpp, the build
// kernels k_image.hip, the scans k_scan.hip's; query.cpp's run_term_batch calls run_image_scan and knows nothing else of this.  Such a scan is bound by the column's
// bytes, and an Int64 / UInt64 column whose values all fit 32 bits carries four bytes per row the comparison does not need.  The column does not
// change between queries — only the constant does — so its truncated copy is made once and every later such scan reads 4 bytes per row through the shipped
// k_scan_cmp<int32 / uint32>, or 2 through the coarse copy.  Both are counted like the decoded form against "hbm_budget_mb" and 80 % of the free HBM.
#include "engine.hpp"
#include "scan_route.hpp"
#include <cstddef>
#include <cstring>

namespace dfdb {
static_assert(CMP_EQ == kCoarseEq && CMP_NE == kCoarseNe && CMP_LT == kCoarseLt && CMP_LE == kCoarseLe && CMP_GT == kCoarseGt && CMP_GE == kCoarseGe, "scan_coarse.hpp numbers the operators as CmpOp does");

// ctx->image_flag, the device words of the two builds (k_image.hip: the image build's `flag`, the coarse build's `hist`)
struct ImageFlag {
  struct Head { uint32_t misfit, max, min; } head;   // a value that does not fit 32 bits was seen; the largest and smallest image value, in unsigned order
  uint8_t pad[256 - sizeof(Head)];
  uint64_t hist[kCoarseHistBins];
};
static_assert(offsetof(ImageFlag, head) == 0 && offsetof(ImageFlag::Head, misfit) == 0 && offsetof(ImageFlag::Head, max) == 4 && offsetof(ImageFlag::Head, min) == 8 &&
              offsetof(ImageFlag, hist) == 256 && sizeof(ImageFlag) == 256 + (size_t)kCoarseHistBins * 8, "k_image.hip's flag words and histogram");

// is there room for `bytes` more beside the table's columns?  (no answer from the device: no)
static bool scan_image_room(dfdb_table* t, size_t bytes) {
  HbmRoom room;
  if (table_hbm_room(t, &room) != hipSuccess) { (void)hipGetLastError(); return false; }
  return (int64_t)bytes <= room.budget && (int64_t)bytes + (64 << 20) <= room.free_now;
}
// The 2-byte coarse copy beside the image just built (scan_coarse.hpp): laid out from the image's min and max, written by one more kernel under its own profile key,
// counted and budgeted like the image.  ctx option "scan_coarse": 1 (default) = made and read, 0 = never made, never read, 2 = read whatever the dense-bucket guard
// says (tests).  No room for it means no coarse copy: the 4-byte image works as before.
static void build_scan_coarse(dfdb_table* t, ScanCopies& sc) {
  dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  if (ctx_option(ctx, "scan_coarse", 1) == 0 || t->nrows <= 0) return;
  const size_t bytes = (size_t)t->nrows * 2 + 256;
  if (!scan_image_room(t, bytes)) { prof_note(ctx, "scan_image.coarse_no_room"); return; }
  try { sc.coarse.ensure(bytes); }
  catch (const Error& e) { if (e.code != DFDB_ERR_NOMEM) throw; (void)hipGetLastError(); sc.coarse.release(); prof_note(ctx, "scan_image.coarse_no_room"); return; }
  const CoarsePlan plan = scan_coarse_plan(sc.min, sc.max);
  sc.shift = plan.shift;
  uint64_t* const hist = ctx->image_flag.as<ImageFlag>()->hist;
  HIP_CHECK(hipMemsetAsync(hist, 0, sizeof(ImageFlag::hist), s));
  { LaunchTimer lt(ctx, "scan_image.coarse_build");
    launch_scan_coarse_build(s, sc.image.p, sc.coarse.p, t->nrows, plan.min, plan.shift, hist); }
  sc.hist.assign((size_t)kCoarseHistBins, 0);
  HIP_CHECK(hipMemcpyAsync(sc.hist.data(), hist, sizeof(ImageFlag::hist), hipMemcpyDeviceToHost, s));
  stream_wait(ctx);                                     // one more wait, once per column (the histogram lands in pageable memory)
  ctx->scan_image_bytes += (int64_t)sc.coarse.bytes;
}
static void build_scan_image(dfdb_table* t, Column& c) {
  dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream; ScanCopies& sc = c.scan;
  const size_t bytes = (size_t)t->nrows * 4 + 256;
  sc.state = kImageNoRoom;
  if (!scan_image_room(t, bytes)) { prof_note(ctx, "scan_image.no_room"); return; }
  try { sc.image.ensure(bytes); ctx->image_flag.ensure(sizeof(ImageFlag)); }
  catch (const Error& e) { if (e.code != DFDB_ERR_NOMEM) throw; (void)hipGetLastError(); sc.image.release(); prof_note(ctx, "scan_image.no_room"); return; }
  uint8_t* const head = ctx->image_flag.as<uint8_t>() + offsetof(ImageFlag, head);
  HIP_CHECK(hipMemsetAsync(head, 0, offsetof(ImageFlag::Head, min), s));                                              // the misfit word and the maximum
  HIP_CHECK(hipMemsetAsync(head + offsetof(ImageFlag::Head, min), 0xff, sizeof(ImageFlag::Head::min), s));
  const bool is_signed = dt_issigned(c.dtype);
  { LaunchTimer lt(ctx, "scan_image.build");
    launch_scan_image_build(s, c.data.p, is_signed, sc.image.p, t->nrows, (uint32_t*)head); }
  // the image is read only after the flag has been: one small copy and one wait, once per column (the min and max words ride in the same copy)
  HIP_CHECK(hipMemcpyAsync(ctx->pinned_scalar, head, sizeof(ImageFlag::Head), hipMemcpyDeviceToHost, s));
  stream_wait(ctx);
  ImageFlag::Head w;
  std::memcpy(&w, ctx->pinned_scalar, sizeof w);
  if (w.misfit != 0) { sc.image.release(); sc.state = kImageMisfit; prof_note(ctx, "scan_image.misfit"); return; }
  sc.state = kImageBuilt;
  ctx->scan_image_bytes += (int64_t)sc.image.bytes;
  const uint32_t unbias = is_signed ? 0x80000000u : 0u;                               // (the kernel reduces the words in unsigned order: k_image.hip image_ordered)
  sc.max = w.max ^ unbias; sc.min = w.min ^ unbias;
  if (w.min <= w.max) build_scan_coarse(t, sc);
}
void drop_scan_image(dfdb_ctx* ctx, Column& c) {
  if (c.scan.image.p) (void)hipStreamSynchronize(ctx->stream);      // a scan that reads it may still be in flight
  ctx->scan_image_bytes -= c.scan.bytes();
  c.scan.clear();
}
// may a lone plain term over this column read the column's copies at all?  (the engine's side of the rule; the constant's is scan_route.hpp's)
static bool scan_image_eligible(const dfdb_table* t, const Column& c, const ScanTerm& tm) {
  return scan_image_dtype(tm.dtype) && !dt_nullable(c.dtype) && dt_base(c.dtype) == tm.dtype && tm.col == c.data.p && !c.comp.p && !c.comp_only && !c.transient && !t->keep_load_scratch;
}
bool run_image_scan(dfdb_query* q, int ord, const ScanTerm& tm, bool have) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const int64_t opt = ctx_option(ctx, "scan_image", 1);
  Column& c = t->cols[(size_t)ord]; ScanCopies& sc = c.scan;
  if (opt == 0 || !scan_image_eligible(t, c, tm)) return false;
  if (sc.scans < INT64_MAX) sc.scans++;
  if (scan_image_builds(sc.state, sc.scans, opt, t->nrows, ctx_option(ctx, "scan_image_min_rows", (int64_t)1 << 24))) build_scan_image(t, c);
  ScanCopyFacts f; f.built = sc.state == kImageBuilt; f.coarse = sc.coarse.p != nullptr; f.min = sc.min; f.max = sc.max; f.shift = sc.shift; f.hist = sc.hist.data(); f.nrows = t->nrows;
  const ScanRoute r = scan_route(tm.dtype, tm.cbits, f, ctx_option(ctx, "scan_coarse", 1));
  if (r.form == kScanFlat) return false;
  LaunchTimer lt(ctx, "scan_image");                   // one launch under this key whatever the form; the notes say which
  const ScanNotes notes = scan_route_notes(r);
  for (int k = 0; k < notes.n; k++) prof_note(ctx, notes.note[k]);
  uint64_t* const bitmap = q->bitmap.as<uint64_t>(); uint32_t* const tile_counts = q->tile_counts.as<uint32_t>(); const int flags = scan_store_flags(ctx);
  const bool exact = r.form == kScanCoarseExact;      // the coarse value is the biased exact value: the shipped 2-byte scan, in its 16-byte-per-lane form
  ScanTerm it = tm; it.col = exact ? sc.coarse.p : sc.image.p; it.dtype = exact ? (int32_t)DFDB_U16 : r.image_dtype; it.cbits = exact ? r.cc : r.image_cbits;
  if (r.form == kScanCoarse) launch_scan_cmp_coarse(s, sc.coarse.p, sc.image.p, r.image_dtype == DFDB_I32, tm.op, r.cc, (uint32_t)r.image_cbits, bitmap, tile_counts, t->nrows, have, (flags & 1) != 0);
  else launch_scan_cmp(s, it, bitmap, tile_counts, t->nrows, have, true, nullptr, exact ? (flags & 1) | (2 << 1) : flags);
  return true;
}

}  // namespace dfdb
