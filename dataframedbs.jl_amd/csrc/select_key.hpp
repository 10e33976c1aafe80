// select_key.hpp — the SELECT KEY of a fixed-width value: an unsigned integer whose order is isless, shared by the radix select (k_select.hip) and the
// radix sort (k_sort.hip).  The key is the order image itself — order_image(value_image(..), value_kind(dtype), false) of value_rules.hpp: integers by value,
// floats -Inf .. -0.0 < 0.0 .. Inf, every NaN last — in 64 bits (FULL), or the same order restated in the 8 * W bits of a W-byte value: the high image bits
// of a narrow type are a function of its own sign bit and carry no order of their own.
#pragma once
#include "device_utils.hpp"
#include "value_rules.hpp"
#include "../../include/dfdb_ir.h"

namespace dfdb {

// the element type a column of base dtype DT is loaded as (Bool is stored as UInt8 and instantiated as DFDB_U8)
template <int DT> struct SelT { using type = uint64_t; };
template <> struct SelT<DFDB_I8> { using type = int8_t; };   template <> struct SelT<DFDB_I16> { using type = int16_t; };
template <> struct SelT<DFDB_I32> { using type = int32_t; }; template <> struct SelT<DFDB_I64> { using type = int64_t; };
template <> struct SelT<DFDB_U8> { using type = uint8_t; };  template <> struct SelT<DFDB_U16> { using type = uint16_t; };
template <> struct SelT<DFDB_U32> { using type = uint32_t; }; template <> struct SelT<DFDB_F32> { using type = float; };
template <> struct SelT<DFDB_F64> { using type = double; };

// how many bits the select key of a column has (Bool is stored as UInt8)
__host__ __device__ constexpr int select_key_bits(int dtype, bool full) {
  if (full) return 64;
  switch (dtype) {
    case DFDB_I8: case DFDB_U8: case DFDB_BOOL: return 8;
    case DFDB_I16: case DFDB_U16: return 16;
    case DFDB_I32: case DFDB_U32: case DFDB_F32: return 32;
    default: return 64;
  }
}
// the select key of the value at `p` (one element of a column of base dtype DT)
template <int DT, bool FULL> __device__ __forceinline__ uint64_t select_key(const void* p) {
  if (FULL || DT == DFDB_I64 || DT == DFDB_U64 || DT == DFDB_F64) return order_image(value_image(p, DT, 0), value_kind(DT), false);
  if (DT == DFDB_F32) {                                                  // Float32 -> Float64 is exact and monotonic: the same order in the float's own bits
    const float f = *(const float*)p;
    const uint32_t b = f32_bits(f);
    return f != f ? 0xffffffffull : (uint64_t)((b >> 31) ? ~b : (b | 0x80000000u));
  }
  if (DT == DFDB_I8) return (uint64_t)(uint8_t)(*(const uint8_t*)p ^ 0x80u);
  if (DT == DFDB_I16) return (uint64_t)(uint16_t)(*(const uint16_t*)p ^ 0x8000u);
  if (DT == DFDB_I32) return (uint64_t)(*(const uint32_t*)p ^ 0x80000000u);
  return value_image(p, DT, 0);                                          // the narrow unsigned types and Bool: the value
}

}  // namespace dfdb
