// scan_coarse.hpp — the 2-byte coarse copy kept beside the 4-byte scan image (scan_image.hpp): how it is laid out, which constants may be compared against it,
// what a coarse comparison decides and when a scan takes it.
// Host-only and free of HIP: tests/scan_coarse_main.cpp compiles it alone with the host compiler under the sanitizers.
//
// The image values x are 32-bit words ordered as the column's type orders them (signed for Int64 columns, unsigned for UInt64 columns).  With min and max the
// smallest and largest of them,
//   span = (uint32)max - (uint32)min       (the modular difference is exact: max >= min in the type's order)
//   shift = max(0, bitlength(span) - 16)
//   coarse(x) = (uint16)(((uint32)x - (uint32)min) >> shift)
// coarse() is monotone over [min, max] and fits 16 bits.  For a constant c inside [min, max] and cc = coarse(c), a row with coarse(x) != cc is decided by the
// two coarse values alone; a row with coarse(x) == cc is undecided when shift > 0 and is compared exactly against the 4-byte image.  With shift == 0 the coarse
// value is the biased exact value and nothing is ever undecided.  A constant outside [min, max] is not folded into "always" / "never": the 4-byte scan runs.
#pragma once
#include <cstdint>
#include "../../include/dfdb_ir.h"

namespace dfdb {

constexpr int kCoarseHistBins = 4096;     // bin k of the build's histogram counts the rows with coarse >> 4 == k
constexpr int64_t kCoarseGuard = 128;     // a refined row moves up to a 64-byte request to save 2 bytes (break-even at 1 row in 32); taken at a four-fold margin under that

struct CoarsePlan { uint32_t min = 0; int32_t shift = 0; };

inline int coarse_bitlength(uint32_t v) { int n = 0; while (v) { n++; v >>= 1; } return n; }

// a <= b in the image type's order
inline bool coarse_le(bool is_signed, uint32_t a, uint32_t b) { return is_signed ? (int32_t)a <= (int32_t)b : a <= b; }

// min, max: the bits of the column's smallest and largest image value
inline CoarsePlan scan_coarse_plan(uint32_t min, uint32_t max) {
  const int bl = coarse_bitlength(max - min);
  CoarsePlan p; p.min = min; p.shift = bl > 16 ? bl - 16 : 0;
  return p;
}
inline uint16_t scan_coarse_value(const CoarsePlan& p, uint32_t x) { return (uint16_t)((x - p.min) >> p.shift); }

// the constant (already an image value: scan_image_const) as the coarse scan takes it; false = outside [min, max], the coarse copy is not used for this scan
inline bool scan_coarse_const(bool is_signed, uint32_t min, uint32_t max, uint32_t c, uint16_t* cc) {
  if (!coarse_le(is_signed, min, c) || !coarse_le(is_signed, c, max)) return false;
  *cc = scan_coarse_value(scan_coarse_plan(min, max), c);
  return true;
}

// the comparison operators as the scan terms number them (kernels.hpp CmpOp; scan_image.cpp asserts that the two agree)
enum : int32_t { kCoarseEq = 0, kCoarseNe = 1, kCoarseLt = 2, kCoarseLe = 3, kCoarseGt = 4, kCoarseGe = 5 };

// what the coarse values decide about x OP c: 0 = false, 1 = true, 2 = undecided (compare image[row] OP c exactly)
inline int scan_coarse_decide(int32_t op, int32_t shift, uint16_t cx, uint16_t cc) {
  if (cx == cc && shift > 0) return 2;
  switch (op) {
    case kCoarseEq: return cx == cc;
    case kCoarseNe: return cx != cc;
    case kCoarseLt: return cx < cc;
    case kCoarseLe: return cx <= cc;
    case kCoarseGt: return cx > cc;
    default:     return cx >= cc;
  }
}

// may a scan whose constant's histogram bin holds bin_rows rows take the coarse form?  (bin_rows * 128 <= nrows, without the product)
inline bool scan_coarse_guard(uint64_t bin_rows, int64_t nrows) { return nrows >= 0 && bin_rows <= (uint64_t)nrows / (uint64_t)kCoarseGuard; }

}  // namespace dfdb
