// scan_image.hpp — the 4-byte scan image of an 8-byte integer column: which columns get one and which constants may be compared against it.
// Host-only and free of HIP: tests/scan_image_const_main.cpp compiles it alone with the host compiler under the sanitizers.
//
// The image of an Int64 column is Int32, of a UInt64 column UInt32: every value truncated, in row order.  It stands for the column only if every value
// equals its truncation extended back (sign extension for Int64, zero extension for UInt64); the build kernel checks that (k_image.hip).  Within that range
// the 4-byte comparison gives the 8-byte comparison's answer exactly when the CONSTANT is in the range too, and that is all this header decides: a constant
// outside it is not folded into "always" / "never" here — the term takes the flat column.
#pragma once
#include <cstdint>
#include "../../include/dfdb_ir.h"

namespace dfdb {

// where a column stands with its image (engine.hpp ScanCopies::state; scan_route.hpp: only kImageNone is ever built from, only kImageBuilt is ever read)
enum : int { kImageNone = 0, kImageBuilt = 1, kImageMisfit = 2 /* some value needs more than 32 bits: never tried again */, kImageNoRoom = 3 /* did not fit the budget */ };
// the image's dtype for a column of base dtype `dtype` (0: this dtype gets no image)
inline int32_t scan_image_dtype(int32_t dtype) { return dtype == DFDB_I64 ? (int32_t)DFDB_I32 : dtype == DFDB_U64 ? (int32_t)DFDB_U32 : 0; }

// does the 8-byte value with these bits equal its truncation extended back in the column's type?
inline bool scan_image_fits(int32_t dtype, uint64_t bits) {
  if (dtype == DFDB_I64) return (uint64_t)(int64_t)(int32_t)(uint32_t)bits == bits;
  if (dtype == DFDB_U64) return (bits >> 32) == 0;
  return false;
}

// the constant of `col OP const` (its bits in the column's own type) as the image's kernel takes it: false = not representable in the image type
inline bool scan_image_const(int32_t dtype, uint64_t cbits, uint64_t* image_cbits) {
  if (!scan_image_fits(dtype, cbits)) return false;
  *image_cbits = cbits & 0xffffffffull;
  return true;
}

}  // namespace dfdb
