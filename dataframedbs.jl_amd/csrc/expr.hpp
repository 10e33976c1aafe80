// expr.hpp — the engine's own reading of the expression IR (include/dfdb_ir.h): typed tree with Julia
// result-type inference (the role Base._return_type plays in src/tables/broadcast.jl:13) and the pattern
// matching that routes a predicate to the specialised scan kernels or to the device interpreter.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

struct dfdb_table;

namespace dfdb {

struct Node {
  int op = 0;
  int32_t dtype = 0;             // inferred result dtype
  int col = -1;                  // DFIR_COL
  uint64_t cbits = 0;            // DFIR_CONST value bit pattern (dtype = const dtype)
  std::string str;               // DFIR_CONST_STR
  std::vector<uint64_t> set;     // DFIR_CONST_SET values (bit patterns of set_dtype)
  int32_t set_dtype = 0;
  int cast_to = 0;
  std::string logical;           // the bits type the Int64 / UInt32 result stands for: "DateTime" for the DFDB_CAST_DATETIME cast, the column's for a DFIR_COL, else empty
  std::unique_ptr<Node> a, b;
  std::unique_ptr<Node> clone() const;
};
using NodePtr = std::unique_ptr<Node>;

// the longest constant of a String coalesce: 1024 rows of it stay far inside the 32-bit selected byte total of a tile (k_str_gather_sizes)
constexpr size_t kMaxCoalesceConst = 65535;
// `coalesce(a, b)` with a String result: a whole projection column (k_strings.hip K6, the two filled forms).  parse_ir admits no other shape: a is a String column leaf, b a
// String column leaf or a string constant
inline bool is_string_coalesce(const Node& n) { return n.op == DFIR_COALESCE && (n.dtype & DFDB_DTYPE_MASK) == DFDB_STRING; }

NodePtr parse_ir(const dfdb_table& t, const uint8_t* ir, size_t len);
NodePtr make_and(NodePtr a, NodePtr b);            // BlockBroadcasting(&, (old, new)): selection.jl:44-47
void required_columns(const Node& n, std::vector<int>& out);  // first-appearance order, unique

int promote_num(int a, int b);

// flatten a tree of DFIR_AND into its conjuncts (left to right)
void flatten_and(const Node& n, std::vector<const Node*>& out);

// `col OP const` / `const OP col` over a numeric column whose constant converts exactly to the column's
// own type; fills term (col pointer left null: the caller resolves the ordinal) and returns the ordinal.
// always: set to +1/-1 when the comparison is constant true/false for every value of the column type.
bool match_simple_term(const Node& n, const dfdb_table& t, ScanTerm& term, int& ordinal);
bool match_column_transform(const Node* e, ScanTerm& out, const Node*& coln);   // the column itself / rem / col * k + d / col / k (ScanTerm::pre)

// `strcol == "x"`, `!=`, startswith, endswith  -> mode 0..3 (launch_str_match)
bool match_string_term(const Node& n, const dfdb_table& t, int& ordinal, int& mode, std::string& pat, bool allow_nullable = false);
// `coalesce(X, false)` with a non-nullable Bool constant false — the way a Union{Bool,Missing} term becomes a predicate — gives X; anything else null
const Node* coalesce_false_arg(const Node& n);
// `s1 OP s2` over two String columns -> their ordinals and the CmpOp (launch_str_pair / launch_dict_pair)
bool match_string_pair_term(const Node& n, int& ord_a, int& ord_b, int& op, bool allow_nullable = false);

}  // namespace dfdb
