// launch_dispatch.hpp — run-time values to compile-time arguments, for the launchers in k_*.hip.  HOST ONLY: a launcher knows a column's base dtype, an
// operator kind or a key's load kind as an int and must name one instantiation of its kernel; each of these switches is written here once.  Not part of
// the interpreter's run-time source (device_utils.hpp and value_rules.hpp are): nothing here may be needed by device code.
#pragma once
#include <cstdint>
#include <type_traits>
#include "../../include/dfdb_ir.h"

namespace dfdb {

// ---- base dtype -> the C++ type of a column's elements.  A launcher lists the cases it has kernels for (they differ: see the lists below); the LAST case of
// a list is its default, as `default:` was in the switches this replaces.  f receives a value of the case's type: `typename decltype(c)::type` is the element
// type, `decltype(c)::dtype` the enumerator (k_select.hip's kernels are instantiated by it).  ALSO: a second enumerator stored the same way (Bool: one UInt8 each)
template <int DT, typename T, int ALSO = DT>
struct DtCase {
  static constexpr int dtype = DT;
  using type = T;
  static constexpr bool matches(int dt) { return dt == DT || dt == ALSO; }
  // the table's unit test.  The three rules are dt_width (common.hpp) and is_signed / is_float (value_rules.hpp) in constant-expression form: those functions
  // are not constexpr, and value_rules.hpp is also the interpreter's run-time source, whose text stays as it is
  static constexpr bool rule_float(int dt) { return dt == DFDB_F32 || dt == DFDB_F64; }
  static constexpr bool rule_signed(int dt) { return dt >= DFDB_I8 && dt <= DFDB_I64; }
  static constexpr int rule_width(int dt) { return dt == DFDB_BOOL ? 1 : (dt == DFDB_F32 ? 4 : (dt == DFDB_F64 ? 8 : 1 << ((dt - DFDB_I8) & 3))); }
  static_assert(DT >= DFDB_I8 && DT <= DFDB_BOOL && ALSO >= DFDB_I8 && ALSO <= DFDB_BOOL, "a fixed-width base dtype");
  static_assert((int)sizeof(T) == rule_width(DT) && (int)sizeof(T) == rule_width(ALSO), "element width");
  static_assert(std::is_floating_point<T>::value == rule_float(DT) && rule_float(ALSO) == rule_float(DT), "float or integer");
  static_assert((std::is_integral<T>::value && std::is_signed<T>::value) == rule_signed(DT) && rule_signed(ALSO) == rule_signed(DT), "signedness");
};
static_assert(DFDB_I8 == 1 && DFDB_I64 == 4 && DFDB_U8 == 5 && DFDB_U64 == 8, "rule_width reads the width off the enumerator: I8 I16 I32 I64 U8 U16 U32 U64");
template <typename... Cases> struct DtList {};

using DtBoolU8 = DtCase<DFDB_U8, uint8_t, DFDB_BOOL>;
// every numeric column and Bool, anything else as Float64: K1's single comparison, the reductions, the order statistics
using DtValues = DtList<DtCase<DFDB_I8, int8_t>, DtCase<DFDB_I16, int16_t>, DtCase<DFDB_I32, int32_t>, DtCase<DFDB_I64, int64_t>, DtBoolU8, DtCase<DFDB_U16, uint16_t>,
                        DtCase<DFDB_U32, uint32_t>, DtCase<DFDB_U64, uint64_t>, DtCase<DFDB_F32, float>, DtCase<DFDB_F64, double>>;
// the numeric columns alone (Bool falls to the default): K3's gather with a transform
using DtNumbers = DtList<DtCase<DFDB_I8, int8_t>, DtCase<DFDB_I16, int16_t>, DtCase<DFDB_I32, int32_t>, DtCase<DFDB_I64, int64_t>, DtCase<DFDB_U8, uint8_t>,
                         DtCase<DFDB_U16, uint16_t>, DtCase<DFDB_U32, uint32_t>, DtCase<DFDB_U64, uint64_t>, DtCase<DFDB_F32, float>, DtCase<DFDB_F64, double>>;
// integer keys and Bool, anything else as UInt64: unique's dense form (unique_dense_dtype says which columns reach it)
using DtDenseKeys = DtList<DtCase<DFDB_I8, int8_t>, DtCase<DFDB_I16, int16_t>, DtCase<DFDB_I32, int32_t>, DtCase<DFDB_I64, int64_t>, DtBoolU8, DtCase<DFDB_U16, uint16_t>,
                           DtCase<DFDB_U32, uint32_t>, DtCase<DFDB_U64, uint64_t>>;

template <typename First, typename... Rest, typename F>
inline void with_dtype_in(DtList<First, Rest...>, int dtype, F& f) {
  if constexpr (sizeof...(Rest) == 0) f(First{});
  else if (First::matches(dtype)) f(First{});
  else with_dtype_in(DtList<Rest...>{}, dtype, f);
}
template <typename List, typename F> inline void with_dtype(int dtype, F&& f) { with_dtype_in(List{}, dtype, f); }

// ---- the 8-byte types: a column of one of them is loaded as it is (the kernels' W8 / V8 / K8 forms; the narrow types go through the dtype switches)
inline bool dt_is_w8(int dtype) { return dtype == DFDB_I64 || dtype == DFDB_U64 || dtype == DFDB_F64; }
// ---- groupreduce's operator kind (k_unique.hip: opk_of — 0 count only, 1 wrapping integer sum, 2 double sum, 3 min, 4 max) -> integral_constant<int, 0..4>
template <typename F>
inline auto with_opk(int opk, F&& f) {
  switch (opk) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}
// can the accumulate kernels with the operator fixed take the value column: there is none to load (count only), or it is 8 bytes wide
inline bool value_is_w8(int opk, int valdt) { return opk == 0 || dt_is_w8(valdt); }

// ---- what a key load is to the radix forms (k_radix.hip): 8 raw bytes (Int64 / UInt64), 8 bytes + isequal's one NaN (Float64), anything narrower (key_image)
enum { kKindRaw8 = 0, kKindF64 = 1, kKindAny = 2 };
template <typename F>
inline auto with_radix_kind(int dtype, F&& f) {
  if (dtype == DFDB_F64) return f(std::integral_constant<int, kKindF64>{});
  if (dtype == DFDB_I64 || dtype == DFDB_U64) return f(std::integral_constant<int, kKindRaw8>{});
  return f(std::integral_constant<int, kKindAny>{});
}

}  // namespace dfdb
