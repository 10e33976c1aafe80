// value_rules.hpp — what a column value MEANS to unique, groupreduce, the aggregates, the casts and parse: each rule once, the same text for the host, the
// kernels and the interpreter's run-time build (jit.cpp compiles this header with hipRTC, as it does device_utils.hpp: no <cmath> / <cstring>, bits move
// through __builtin_memcpy, a NaN is x != x).  dtype arguments are base dtypes (no DFDB_NULLABLE bit).  tests/test_value_rules_cpu.py pins the host side bit
// for bit through dfdb_selftest("value_rules"); tests/test_gpu_value_rules.py carries the same edge values through every device form.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/dfdb_ir.h"
#endif

namespace dfdb {

__host__ __device__ __forceinline__ bool is_float(int dtype) { return dtype == DFDB_F32 || dtype == DFDB_F64; }
__host__ __device__ __forceinline__ bool is_signed(int dtype) { return dtype >= DFDB_I8 && dtype <= DFDB_I64; }

// bit moves (the fixed-width reinterpretations __float_as_uint / __double_as_longlong / __longlong_as_double, for the host too)
__host__ __device__ __forceinline__ uint32_t f32_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
__host__ __device__ __forceinline__ uint64_t f64_bits(double d) { uint64_t u; __builtin_memcpy(&u, &d, 8); return u; }
__host__ __device__ __forceinline__ double bits_f64(uint64_t u) { double d; __builtin_memcpy(&d, &u, 8); return d; }

// ---- accumulator kinds: the 64 bits a sum / min / max works on are an Int64 (wrapping sum, signed order), a UInt64 or a Float64 (Float32 widened)
enum { kAccSigned = 0, kAccUnsigned = 1, kAccFloat = 2 };
__host__ __device__ __forceinline__ int value_kind(int dtype) {
  switch (dtype) {
    case DFDB_I8: case DFDB_I16: case DFDB_I32: case DFDB_I64: return kAccSigned;
    case DFDB_U8: case DFDB_BOOL: case DFDB_U16: case DFDB_U32: case DFDB_U64: return kAccUnsigned;
    default: return kAccFloat;
  }
}
__host__ __device__ __forceinline__ int kind_dtype(int kind) { return kind == kAccFloat ? DFDB_F64 : (kind == kAccUnsigned ? DFDB_U64 : DFDB_I64); }   // the dtype an accumulator's 64 bits are returned as

// ---- 64-bit image of row `row` of a fixed-width column under isequal (Base.isequal: NaN == NaN whatever the payload, 0.0 != -0.0): integers by value,
// floats by their bits with ONE NaN per width
__host__ __device__ __forceinline__ uint64_t key_image(const void* col, int dtype, int64_t row) {
  switch (dtype) {
    case DFDB_I8:  return (uint64_t)(int64_t)((const int8_t*)col)[row];
    case DFDB_I16: return (uint64_t)(int64_t)((const int16_t*)col)[row];
    case DFDB_I32: return (uint64_t)(int64_t)((const int32_t*)col)[row];
    case DFDB_U8: case DFDB_BOOL: return ((const uint8_t*)col)[row];
    case DFDB_U16: return ((const uint16_t*)col)[row];
    case DFDB_U32: return ((const uint32_t*)col)[row];
    case DFDB_F32: { const float f = ((const float*)col)[row]; return f != f ? 0x7fc00000ull : (uint64_t)f32_bits(f); }
    case DFDB_F64: { const double d = ((const double*)col)[row]; return d != d ? 0x7ff8000000000000ull : f64_bits(d); }
    default: return ((const uint64_t*)col)[row];
  }
}
// ---- the value of row `row` as the 64 bits its accumulator (value_kind) works on: integers widened, Float32 as the double it converts to
__host__ __device__ __forceinline__ uint64_t value_image(const void* col, int dtype, int64_t row) {
  switch (dtype) {
    case DFDB_I8:  return (uint64_t)(int64_t)((const int8_t*)col)[row];
    case DFDB_I16: return (uint64_t)(int64_t)((const int16_t*)col)[row];
    case DFDB_I32: return (uint64_t)(int64_t)((const int32_t*)col)[row];
    case DFDB_U8: case DFDB_BOOL: return ((const uint8_t*)col)[row];
    case DFDB_U16: return ((const uint16_t*)col)[row];
    case DFDB_U32: return ((const uint32_t*)col)[row];
    case DFDB_F32: return f64_bits((double)((const float*)col)[row]);
    default: return ((const uint64_t*)col)[row];
  }
}
// ---- order-preserving image of an accumulator's bits for an atomic min / max under UNSIGNED compare; a NaN maps to the end that wins the reduction
// (Julia's minimum / maximum propagate NaN)
__host__ __device__ __forceinline__ uint64_t order_image(uint64_t bits, int kind, bool is_min) {
  if (kind == kAccUnsigned) return bits;
  if (kind == kAccSigned) return bits ^ (1ull << 63);
  const double d = bits_f64(bits);
  if (d != d) return is_min ? 0ull : ~0ull;
  return (bits >> 63) ? ~bits : (bits | (1ull << 63));
}
// ---- Julia's min / max on Float64 (Base.min / Base.max, math.jl): a NaN operand is the result, and -0.0 orders below 0.0.  Equal values share their bits
// except the two zeros — OR keeps a sign bit either of them has, AND drops one either lacks — so the result does not depend on which zero came first
// (`b < a ? b : a` did: minimum() of a column holding 0.0 and -0.0 depended on the grid; found by the block-streamed aggregates, round 6)
__host__ __device__ __forceinline__ double minmax_f64(double a, double b, bool is_min) {
  if (a != a) return a;
  if (b != b) return b;
  if (a == b) { const uint64_t x = f64_bits(a), y = f64_bits(b); return bits_f64(is_min ? (x | y) : (x & y)); }
  if (is_min) return b < a ? b : a;
  return b > a ? b : a;
}
// ---- what a reduction starts from, per accumulator type A (int64_t / uint64_t / double); neither is_min nor is_max: a sum
template <typename A> __host__ __device__ __forceinline__ A reduce_identity(bool is_min, bool is_max);
template <> __host__ __device__ __forceinline__ int64_t reduce_identity<int64_t>(bool is_min, bool is_max) { return is_min ? 9223372036854775807LL : (is_max ? -9223372036854775807LL - 1 : 0); }
template <> __host__ __device__ __forceinline__ uint64_t reduce_identity<uint64_t>(bool is_min, bool) { return is_min ? ~0ull : 0ull; }
template <> __host__ __device__ __forceinline__ double reduce_identity<double>(bool is_min, bool is_max) { return is_min ? __builtin_inf() : (is_max ? -__builtin_inf() : 0.0); }
// the same as the 64 bits of an accumulator of kind `kind`
__host__ __device__ __forceinline__ uint64_t reduce_identity_bits(int kind, bool is_min, bool is_max) {
  if (kind == kAccFloat) return f64_bits(reduce_identity<double>(is_min, is_max));
  if (kind == kAccSigned) return (uint64_t)reduce_identity<int64_t>(is_min, is_max);
  return reduce_identity<uint64_t>(is_min, is_max);
}

// ---- typemin / typemax of the integer dtypes (anything else reads as UInt64) and `x % T`, the wrap of a 64-bit image to a narrow integer type
__host__ __device__ __forceinline__ int64_t int_lo(int dtype) {
  switch (dtype) { case DFDB_I8: return -128; case DFDB_I16: return -32768; case DFDB_I32: return -2147483648LL; case DFDB_I64: return -9223372036854775807LL - 1; }
  return 0;
}
__host__ __device__ __forceinline__ uint64_t int_hi(int dtype) {
  switch (dtype) {
    case DFDB_I8: return 127; case DFDB_I16: return 32767; case DFDB_I32: return 2147483647ull; case DFDB_I64: return 9223372036854775807ull;
    case DFDB_U8: return 255; case DFDB_U16: return 65535; case DFDB_U32: return 4294967295ull;
    default: return ~0ull;
  }
}
__host__ __device__ __forceinline__ int64_t wrap_int(int64_t x, int dtype) {
  switch (dtype) {
    case DFDB_I8: return (int8_t)x; case DFDB_I16: return (int16_t)x; case DFDB_I32: return (int32_t)x;
    case DFDB_U8: return (uint8_t)x; case DFDB_U16: return (uint16_t)x; case DFDB_U32: return (uint32_t)x;
    default: return x;
  }
}

}  // namespace dfdb
