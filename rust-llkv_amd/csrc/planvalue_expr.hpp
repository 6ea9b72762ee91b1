// planvalue_expr.hpp — conditional expressions in GROUP BY aggregate arguments, host side: the static check of a token program
// (shape, caps, and which class may stand where: the refusals that need no column statistics), made once for the plan lowering
// (plan.cpp: expr_planvalue) and the host evaluator, and the evaluator of one row (llkv_hip_scalar_eval_planvalue) over the
// rules of planvalue_rules.h.  No device, no engine state.
#pragma once

#include "llkv_hip.h"
#include "planvalue_rules.h"

#include <functional>
#include <string>
#include <vector>

namespace llkv {

// does the program use a conditional token kind (LLKV_TOK_COMPARE …, LLKV_BIN_AND / LLKV_BIN_OR)?
bool cond_program(const llkv_expr_token *e, uint32_t n);
// what every consumer of token programs other than GROUP BY aggregate arguments answers for such a program
int cond_refuse_elsewhere(const llkv_expr_token *e, uint32_t n, const char *where, std::string *err);

// the PvClass of a column's values from its dtype; kPvDecimal for Decimal128, −1 for a dtype no program takes
int cond_class_of_dtype(int32_t dtype);

enum CondOrigin : uint8_t { kCondComputed = 0, kCondColumn = 1, kCondLiteral = 2 };
struct CondNode { // the value a token pushes
  int cls = kPvNull;      // PvClass; kPvNull: the NULL literal only
  uint8_t origin = kCondComputed;
};
// field id → PvClass of the column (cond_class_of_dtype), −2: no such field
using CondLeafClass = std::function<int(uint32_t field_id)>;

// LLKV_OK and nodes[i] for every token, or the refusal: LLKV_INVALID_ARGUMENT for a malformed program, LLKV_UNSUPPORTED beyond a
// cap or for a class the rules do not serve where it stands, LLKV_NOT_FOUND for an unknown field; the message names the token.
int cond_static_check(const llkv_expr_token *e, uint32_t n, const CondLeafClass &leaf, std::vector<CondNode> *nodes, std::string *err);

// One row.  A cell: the class of its column, and its value unless NULL.
struct CondCell {
  int cls = kPvInteger;
  bool is_null = true;
  int64_t i = 0;   // Integer; Date32: days
  double f = 0.0;  // Float
  std::string s;   // String
};
struct CondValue { // Null, Integer or Float
  int cls = kPvNull;
  int64_t i = 0;
  double f = 0.0;
};
using CondCellOf = std::function<const CondCell *(uint32_t field_id)>; // nullptr: no such field
int cond_eval_row(const llkv_expr_token *e, uint32_t n, const CondCellOf &cell, CondValue *out, std::string *err);

} // namespace llkv
