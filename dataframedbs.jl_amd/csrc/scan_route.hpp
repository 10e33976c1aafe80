// scan_route.hpp — which form a lone `col OP const` scan of an Int64 / UInt64 column takes, given the copies the column holds (engine.hpp ScanCopies): the flat
// column, its 4-byte image (scan_image.hpp), or the 2-byte coarse copy beside the image (scan_coarse.hpp) — and when a scan builds the image.  DESIGN.md §3.
// Host-only and free of HIP: tests/scan_route_main.cpp compiles it alone with the host compiler under the sanitizers.  scan_image.cpp acts on what it says.
#pragma once
#include "scan_image.hpp"
#include "scan_coarse.hpp"

namespace dfdb {

// does this scan — the column's `scans`-th that could read an image — build it?  opt: ctx option "scan_image" (0 = never built, never read; 1 = the SECOND such
// scan builds: a one-off query never pays, the build moves 12 bytes per row and a scan saves 4; 2 = the first does), min_rows: "scan_image_min_rows" (a scan
// below it is launch-bound).  A column that did not fit 32 bits, or the budget, is not tried again until it is reloaded.
inline bool scan_image_builds(int state, int64_t scans, int64_t opt, int64_t nrows, int64_t min_rows) {
  return opt != 0 && state == kImageNone && (opt == 2 || scans >= 2) && nrows >= min_rows;
}

// what the column's copies are, as the rule needs them (min, max, shift, hist mean something only beside built / coarse)
struct ScanCopyFacts {
  bool built = false, coarse = false;   // the image stands for the column; it has a coarse copy
  uint32_t min = 0, max = 0;            // the bits of the smallest and largest image value
  int32_t shift = 0;                    // the coarse copy's
  const uint64_t* hist = nullptr;       // kCoarseHistBins words: rows whose coarse value >> 4 is k
  int64_t nrows = 0;
};

enum ScanForm : int {
  kScanFlat = 0,         // the 8-byte column: no image, or a constant the image type cannot hold (nothing is folded into "always" / "never")
  kScanImage,            // k_scan_cmp over the 4-byte image
  kScanCoarseExact,      // shift 0, the coarse value is the biased exact value: k_scan_cmp over the 2-byte copy
  kScanCoarse            // k_scan_cmp_coarse: 2 bytes per row, the rows in the constant's bucket refined from the image
};
struct ScanRoute {
  int form = kScanFlat;
  bool dense = false;          // kScanImage because the constant's bucket is a dense one: every row of it would be refined
  int32_t image_dtype = 0;     // DFDB_I32 / DFDB_U32 (every form but flat)
  uint64_t image_cbits = 0;    // the constant truncated to the image type
  uint16_t cc = 0;             // the constant's coarse value (the coarse forms and dense)
};

// coarse_opt: ctx option "scan_coarse" (0 = the coarse copy is never read, 1 = read unless the dense-bucket guard refuses, 2 = read whatever the guard says)
inline ScanRoute scan_route(int32_t dtype, uint64_t cbits, const ScanCopyFacts& f, int64_t coarse_opt) {
  ScanRoute r;
  uint64_t cb = 0;
  if (!f.built || !scan_image_dtype(dtype) || !scan_image_const(dtype, cbits, &cb)) return r;
  r.form = kScanImage; r.image_dtype = scan_image_dtype(dtype); r.image_cbits = cb;
  // the 2-byte copy where the column has one and the constant lies inside the column's [min, max]
  if (coarse_opt == 0 || !f.coarse || !scan_coarse_const(r.image_dtype == DFDB_I32, f.min, f.max, (uint32_t)cb, &r.cc)) return r;
  if (f.shift == 0) r.form = kScanCoarseExact;
  else if (coarse_opt == 2 || scan_coarse_guard(f.hist[r.cc >> 4], f.nrows)) r.form = kScanCoarse;
  else r.dense = true;
  return r;
}

// the profile notes the routed scan leaves, in order (the flat scan's are its own: query.cpp)
struct ScanNotes { int n; const char* note[2]; };
inline ScanNotes scan_route_notes(const ScanRoute& r) {
  const char* const image = r.image_dtype == DFDB_I32 ? "scan_image.int32" : "scan_image.uint32";
  switch (r.form) {
    case kScanCoarseExact: return ScanNotes{1, {"scan_image.coarse_exact", nullptr}};
    case kScanCoarse:      return ScanNotes{1, {"scan_image.coarse", nullptr}};
    case kScanImage:       return r.dense ? ScanNotes{2, {"scan_image.coarse_dense", image}} : ScanNotes{1, {image, nullptr}};
    default:               return ScanNotes{0, {nullptr, nullptr}};
  }
}

}  // namespace dfdb
