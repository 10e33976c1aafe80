/* dfdb_ir.h — predicate / computed-column expression IR shared by every front-end.
 *
 * The reference expresses predicates and computed columns as a tree of
 * `BlockBroadcasting{RT,F,Args}` nodes whose leaves are `ColRef{T}` or 0-dim
 * scalars (reference: src/tables/broadcast.jl:2-17) and JIT-fuses any Julia
 * function over them (broadcast.jl:60-68).  A C ABI cannot carry closures, so
 * the tree is serialised as a little-endian POSTFIX byte stream over the closed
 * operator set the reference's tests and docs exercise.
 *
 *   stream := token*            (evaluation leaves exactly one value on the stack)
 *   token  := opcode:u8 payload
 *
 * Result types are NOT carried: every consumer infers them with Julia's
 * promotion rules (see DESIGN.md "IR typing"), the same way the reference gets
 * RT from Base._return_type (broadcast.jl:13).
 */
#ifndef DFDB_IR_H
#define DFDB_IR_H

/* ---- column / scalar dtypes (ColumnTypes names: src/columntypes/base.jl:108-126) ---- */
enum {
  DFDB_I8 = 1, DFDB_I16 = 2, DFDB_I32 = 3, DFDB_I64 = 4,
  DFDB_U8 = 5, DFDB_U16 = 6, DFDB_U32 = 7, DFDB_U64 = 8,
  DFDB_F32 = 9, DFDB_F64 = 10, DFDB_BOOL = 11, DFDB_STRING = 12,
  DFDB_DTYPE_MASK = 0x3f,
  DFDB_NULLABLE = 0x80, /* Union{T,Missing}: "Missing(T)" on disk */
  /* not a dtype: a cast TARGET, valid only as the payload byte of DFIR_CAST over a String column leaf (see DFIR_CAST below).  Bit 0x40 lies outside
   * DFDB_DTYPE_MASK, so `target & DFDB_DTYPE_MASK` reads Int64, the representation of the result: every consumer tests for the whole byte first. */
  DFDB_CAST_DATETIME = 0x40 | DFDB_I64
};

/* ---- leaves ---- */
#define DFIR_COL        0x01 /* payload: u32 column ordinal (0-based position in the table) */
#define DFIR_CONST      0x02 /* payload: u8 dtype, 8 bytes (value bit pattern, zero/sign extended) */
#define DFIR_CONST_STR  0x03 /* payload: u32 nbytes, bytes (Julia: "x" / Ref("x")) */
#define DFIR_CONST_SET  0x04 /* payload: u8 dtype, u32 n, n*8 bytes (Julia: Ref([..]) for in.()) */

/* ---- arithmetic (binary unless noted) ---- */
#define DFIR_ADD   0x10
#define DFIR_SUB   0x11
#define DFIR_MUL   0x12
#define DFIR_DIV   0x13 /* Julia `/`  : integers -> Float64 */
#define DFIR_IDIV  0x14 /* Julia `÷`  : truncating, DivideError on 0 */
#define DFIR_REM   0x15 /* Julia `%`  : sign of dividend, DivideError on 0 */
#define DFIR_MOD   0x16 /* Julia mod(): sign of divisor */
#define DFIR_NEG   0x17 /* unary */
#define DFIR_ABS   0x18 /* unary */
#define DFIR_MIN   0x19
#define DFIR_MAX   0x1a

/* ---- comparisons -> Bool (Int vs Float compared exactly, like Julia) ---- */
#define DFIR_EQ    0x20
#define DFIR_NE    0x21
#define DFIR_LT    0x22
#define DFIR_LE    0x23
#define DFIR_GT    0x24
#define DFIR_GE    0x25
/* String OP String is Base.cmp(::String, ::String) on the bytes: memcmp over the common prefix, then the lengths, bytes unsigned ("\xff" > "\x7f", a proper
 * prefix is smaller, an embedded NUL is a byte like any other).  Either operand may be a String column or a string constant (at least one is a column); with a
 * Union{String,Missing} operand the result is Union{Bool,Missing}, missing where either side is — as a predicate it needs coalesce(s1 OP s2, false).
 * startswith / endswith take a constant pattern only. */

/* ---- logic: Bool (non-short-circuit, like `&` in selection.jl:46) or bitwise on ints ---- */
#define DFIR_AND   0x30
#define DFIR_OR    0x31
#define DFIR_XOR   0x32
#define DFIR_NOT   0x33 /* unary `!` */

/* ---- set / string / missing ---- */
#define DFIR_IN_SET      0x40 /* stack: value, set        -> Bool   (in.(a, Ref(v)), numeric sets; a set of strings is lowered by the front ends to (a == v1) | (a == v2) | ...) */
#define DFIR_STARTSWITH  0x41 /* stack: string col, const -> Bool */
#define DFIR_ENDSWITH    0x42
#define DFIR_ISMISSING   0x43 /* unary on a nullable column -> Bool */
#define DFIR_SIZEOF      0x44 /* unary: sizeof(string) -> Int64 */
#define DFIR_COALESCE    0x45 /* binary: coalesce(a, b) = a unless it is missing, else b (same base type; result nullable iff b is) */
/* DFIR_COALESCE over numeric operands takes any expressions.  Over Strings it makes a computed String column (the tutorial's string_convert,
 * docs/src/index.md:437-453, and string(missing) at :424) and takes two leaves only:
 *   a        a String or Union{String,Missing} COLUMN leaf
 *   b        a string constant (DFIR_CONST_STR, at most 65535 bytes) or a String / Union{String,Missing} COLUMN leaf of the same table
 *   row i    a[i] where a[i] is not missing, else b[i] (or the constant); no row raises
 *   type     String; Union{String,Missing} iff b is a nullable column — a row missing on both sides stays missing (size -1, no bytes).  Over a
 *            non-nullable a the result equals column a
 * The expression is valid only as a WHOLE projection column (dfdb_result_string_bytes, dfdb_materialize, dfdb_table_add_from_query, resident, streamed
 * and sharded).  Everything else is DFDB_ERR_UNSUPPORTED: a String coalesce as an operand of any operation (a comparison, sizeof, parse, startswith, a
 * second coalesce) or as a predicate, any other operand shape, a longer constant; coalesce(String, number) is refused as a Union of two value types;
 * unique / groupreduce over it keep their refusal of computed columns — dfdb_table_add_from_query makes it a column first. */

/* ---- conversion ---- */
#define DFIR_CAST  0x50 /* payload: u8 dtype ; Julia T(x) / convert */
/* DFIR_CAST applied to a String operand means parse(T, s) (Julia has no T("12"), so `COL s; CAST T` is free: "convert this column to T").
 *   operand  a String or Union{String,Missing} COLUMN leaf, as for sizeof; any other String-typed operand is DFDB_ERR_UNSUPPORTED
 *   targets  Int8 .. Int64, UInt8 .. UInt64, Float64 (Bool, Float32, String: DFDB_ERR_UNSUPPORTED)
 *   type     the target, never Union{T,Missing}, also over a nullable column: parse(T, ::Missing) is a MethodError
 * Integers are the ASCII subset of Base.tryparse_internal: [ws][+-]digits[ws], ws = 0x20 and 0x09-0x0d, `-` for signed targets only; leading zeros are
 * fine, "-9223372036854775808" parses, "-0" is 0.  Every evaluated row ends in exactly one of three ways:
 *   1. the value;
 *   2. an error Julia certainly raises too, status DFDB_ERR_ARGUMENT with the smallest raising row, the message starts with the Julia name:
 *        "ArgumentError:"  empty or all whitespace, a sign with nothing after it, a non-digit where a digit must be, characters after trailing
 *                          whitespace, `-` with an unsigned target
 *        "OverflowError:"  the value does not fit the target (read left to right: whichever of the two comes first in the string)
 *        "MethodError: no method matching parse(::Type{T}, ::Missing)"  a missing row
 *   3. DFDB_ERR_UNSUPPORTED with the row, "the caller falls back to the Julia path": strings Julia may accept and the device does not try — any byte
 *      >= 0x80 (Unicode spaces), whitespace directly after the sign, digits that start 0x / 0o / 0b.  Never reported as ArgumentError, never given a value.
 * Float64 is the correctly rounded value or DFDB_ERR_UNSUPPORTED, never an approximation: [ws][+-](digits[.digits*] | .digits)[(e|E)[+-]digits][ws] whose
 * significand with the point removed is < 2^53 and whose power of ten then has |e10| <= 22 — one IEEE multiply or divide of two exact doubles (Clinger's
 * fast path; "35.79" is 3579 / 1e2, "-0.0" keeps its sign).  Longer significands, larger exponents, Inf, NaN, hex floats, "1f3", underscores: UNSUPPORTED
 * with the smallest such row; empty, all-whitespace and missing rows raise as for integers.
 * Which rows count as evaluated, and which of several errors is reported (the smallest row among all kinds), follows the rule of DivideError / InexactError. */
/* DFIR_CAST with the target DFDB_CAST_DATETIME over a String or Union{String,Missing} COLUMN leaf (the same operand restriction as parse; over any other
 * operand the target is DFDB_ERR_UNSUPPORTED) is the timestamp conversion of the reference's tutorial (docs/src/index.md:417-435), spelled datetime19(s)
 * by the front ends: string(s) is cut at the fixed character ranges 1:4, 6:7, 9:10, 12:13, 15:16, 18:19, each piece is parsed as Int64, and the six numbers
 * are the arguments of DateTime(y, m, d, h, mi, s).  Result: DFDB_I64, never nullable, logical type "DateTime" (milliseconds, Dates' Rata Die epoch).
 * This is the tutorial's function and NOT DateTime(s): the bytes at 4, 7, 10, 13, 16 and everything from byte 19 on are ignored, so
 * "2019-10-01 00:00:00 UTC", "2019-10-01T00:00:00" and "2019-10-01T00:00:00.123" all give 2019-10-01T00:00:00.  With n = sizeof(s), every evaluated row
 * is settled by the FIRST rule that applies:
 *   1. the row is missing (string(missing) is 7 bytes long), or n < 19 and the bytes [0, n) are all < 0x80: status DFDB_ERR_BOUNDS, the message starts
 *      with "BoundsError:" (SubString raises before any field is parsed);
 *   2. a byte >= 0x80 among the first min(n, 19): DFDB_ERR_UNSUPPORTED (character indices stop being byte indices: Julia decides);
 *   3. one of the 14 field bytes (0-3, 5-6, 8-9, 11-12, 14-15, 17-18) is not '0'..'9': DFDB_ERR_UNSUPPORTED (parse(Int64, " 1"), "+1" and "0x1f" are
 *      values in Julia and "1a" is not; the device does not sort them out);
 *   4. month outside 1:12; else day outside 1:daysinmonth(y, m) (proleptic Gregorian leap rule, year 0000 is a leap year); else hour 25..99; else, the
 *      hour being below 24, minute >= 60; else second >= 60: status DFDB_ERR_ARGUMENT, the message starts with "ArgumentError: DateTime:";
 *   5. hour == 24 (month and day in range), whatever minute and second are: DFDB_ERR_UNSUPPORTED (Julia versions differ on DateTime(y, m, d, 24));
 *   6. otherwise the value 1000 * (s + 60 mi + 3600 h + 86400 * totaldays(y, m, d)), totaldays as in Dates with floored divisions:
 *        z = m < 3 ? y - 1 : y;  totaldays = d + SHIFT[m] + 365 z + fld(z, 4) - fld(z, 100) + fld(z, 400) - 306
 *        SHIFT = (306, 337, 0, 31, 61, 92, 122, 153, 184, 214, 245, 275)
 *      ("1970-01-01 00:00:00" is 62135683200000; "0000-01-01 00:00:00" is -31536000000, totaldays = -365).
 * Which rows count as evaluated, and which of several raising rows is reported, is parse's rule: the smallest row of any kind, only selected rows, and the
 * converted leaf wins a tie on its row. */

#endif
