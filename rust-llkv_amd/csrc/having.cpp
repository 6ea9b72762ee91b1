// having.cpp — HAVING over the output cells of a GROUP BY, host side: the owned program, its validation and THE host evaluator
// (evaluate_having_expr llkv-executor/src/lib.rs:6667-7006; value expressions as operands :7177-7516).  llkv_hip_having_eval(_ex)
// and GroupResult::apply both run having_eval;
// the numeric rules it applies are those of having_rules.h, which the device flag kernel (group_having.hip) applies too.
#include "engine.hpp"
#include "having_rules.h"

#include <cstring>

namespace llkv {

namespace {

const char *kind_name(int32_t kind) {
  switch (kind) {
  case LLKV_HAVING_COMPARE: return "COMPARE";
  case LLKV_HAVING_IN_LIST: return "IN_LIST";
  case LLKV_HAVING_IS_NULL: return "IS_NULL";
  case LLKV_HAVING_LITERAL: return "LITERAL";
  case LLKV_HAVING_AND: return "AND";
  case LLKV_HAVING_OR: return "OR";
  case LLKV_HAVING_NOT: return "NOT";
  default: return "?";
  }
}

const char *token_name(int32_t op) {
  switch (op) {
  case LLKV_HAVING_TOKEN_PUSH: return "PUSH";
  case LLKV_HAVING_TOKEN_ADD: return "ADD";
  case LLKV_HAVING_TOKEN_SUB: return "SUB";
  case LLKV_HAVING_TOKEN_MUL: return "MUL";
  case LLKV_HAVING_TOKEN_DIV: return "DIV";
  case LLKV_HAVING_TOKEN_MOD: return "MOD";
  case LLKV_HAVING_TOKEN_SHL: return "SHL";
  case LLKV_HAVING_TOKEN_SHR: return "SHR";
  case LLKV_HAVING_TOKEN_CAST_INT: return "CAST_INT";
  case LLKV_HAVING_TOKEN_CAST_FLOAT: return "CAST_FLOAT";
  case LLKV_HAVING_TOKEN_COALESCE: return "COALESCE";
  default: return "?";
  }
}

std::string node_name(uint32_t i, int32_t kind) { return "HAVING node " + std::to_string(i) + " (" + kind_name(kind) + ")"; }

// plan_value_from_literal as evaluate_expr_with_plan_value_aggregates_and_row applies it (:7019-7028)
HavingValue literal_value(const llkv_literal &l, const char **str) {
  *str = nullptr;
  switch (l.tag) {
  case LLKV_LIT_INT128: return {kHvInteger, l.lo}; // `as i64`: the low 64 bits
  case LLKV_LIT_BOOLEAN: return {kHvInteger, l.lo ? 1u : 0u};
  case LLKV_LIT_FLOAT64: { uint64_t b; std::memcpy(&b, &l.f64, 8); return {kHvFloat, b}; }
  case LLKV_LIT_DECIMAL128: return {kHvDecimal, 0};
  case LLKV_LIT_STRING: *str = l.str ? l.str : ""; return {kHvString, 0};
  case LLKV_LIT_DATE32: return {kHvDate32, 0};
  default: return {kHvNull, 0};
  }
}

// plan_value_from_array (llkv-plan/src/plans.rs:1131-1197) of a finalized cell.  `column_dtype`: a key cell is typed by its
// COLUMN (GroupResult::cell_key hands Date32 and Boolean cells over as LLKV_DT_INT64); < 0: an aggregate cell, typed by itself.
HavingValue cell_value(const llkv_value &v, int32_t column_dtype, const char **str) {
  *str = nullptr;
  if (v.is_null) return {kHvNull, 0};
  switch (column_dtype >= 0 ? column_dtype : v.dtype) {
  case LLKV_DT_FLOAT64: case LLKV_DT_FLOAT32: { uint64_t b; std::memcpy(&b, &v.f64, 8); return {kHvFloat, b}; }
  case LLKV_DT_DECIMAL128: return {kHvDecimal, 0};
  case LLKV_DT_UTF8: *str = v.str ? v.str : ""; return {kHvString, 0};
  case LLKV_DT_DATE32: return {kHvDate32, 0};
  case LLKV_DT_BOOLEAN: return {kHvInteger, v.i64 ? 1u : 0u};
  case LLKV_DT_NULL: return {kHvNull, 0};
  default: return {kHvInteger, (uint64_t)v.i64}; // Int64 (and the narrower integer key columns this library groups by)
  }
}

int leaf_value(const llkv_having_operand &o, const HavingCell &cell, HavingValue *out, const char **str);

// An expression operand: its tokens over the value stack, by the rules of having_rules.h (the flag kernel runs the same).
int expr_value(const llkv_having_expr &e, const HavingCell &cell, HavingValue *out) {
  HavingValueStack st;
  for (uint32_t t = 0; t < e.n_tokens; ++t) {
    const llkv_having_token &tk = e.tokens[t];
    if (tk.op != LLKV_HAVING_TOKEN_PUSH) { having_token(st, tk.op, tk.arg); continue; }
    HavingValue v;
    const char *str;
    if (int rc = leaf_value(tk.leaf, cell, &v, &str)) return rc;
    if (v.tag != kHvNull && v.tag != kHvInteger && v.tag != kHvFloat)
      return set_error(LLKV_UNSUPPORTED, std::string("HAVING expression token ") + std::to_string(t) + " (PUSH): a " +
                                             (v.tag == kHvString ? "Utf8" : v.tag == kHvDecimal ? "Decimal128" : "Date32") + " value inside an expression");
    st.push(v);
  }
  *out = st.pop();
  return LLKV_OK;
}

struct ExprTable {
  const llkv_having_expr *exprs;
  uint32_t n;
};

int operand_value(const llkv_having_operand &o, const ExprTable &x, const HavingCell &cell, HavingValue *out, const char **str) {
  if (o.kind != LLKV_HAVING_OPERAND_EXPR) return leaf_value(o, cell, out, str);
  *str = nullptr;
  return expr_value(x.exprs[o.index], cell, out);
}

int leaf_value(const llkv_having_operand &o, const HavingCell &cell, HavingValue *out, const char **str) {
  if (o.kind == LLKV_HAVING_OPERAND_LITERAL) { *out = literal_value(o.literal, str); return LLKV_OK; }
  llkv_value v;
  int32_t key_dtype = -1;
  if (int rc = cell(o, &v, &key_dtype)) return rc;
  *out = cell_value(v, o.kind == LLKV_HAVING_OPERAND_KEY ? key_dtype : -1, str);
  return LLKV_OK;
}

int check_expr(const llkv_having_expr &e, const std::string &ex, uint32_t n_keys, uint32_t n_aggs, std::string *err);

int check_operand(const llkv_having_operand &o, uint32_t n_keys, uint32_t n_aggs, const ExprTable &x, const std::string &where, std::string *err) {
  switch (o.kind) {
  case LLKV_HAVING_OPERAND_EXPR:
    if (o.index >= x.n) { *err = where + ": expression index " + std::to_string(o.index) + " is out of range for " + std::to_string(x.n) + " expressions"; return LLKV_INVALID_ARGUMENT; }
    return check_expr(x.exprs[o.index], where + " expression " + std::to_string(o.index), n_keys, n_aggs, err);
  case LLKV_HAVING_OPERAND_KEY:
    if (o.index >= n_keys) { *err = where + ": key index " + std::to_string(o.index) + " is out of range for " + std::to_string(n_keys) + " keys"; return LLKV_INVALID_ARGUMENT; }
    return LLKV_OK;
  case LLKV_HAVING_OPERAND_AGGREGATE:
    if (o.index >= n_aggs) { *err = where + ": aggregate index " + std::to_string(o.index) + " is out of range for " + std::to_string(n_aggs) + " aggregates"; return LLKV_INVALID_ARGUMENT; }
    return LLKV_OK;
  case LLKV_HAVING_OPERAND_LITERAL:
    if (o.literal.tag < LLKV_LIT_NULL || o.literal.tag > LLKV_LIT_DATE32) { *err = where + ": unknown literal tag " + std::to_string(o.literal.tag); return LLKV_INVALID_ARGUMENT; }
    return LLKV_OK;
  default: *err = where + ": unknown operand kind " + std::to_string(o.kind); return LLKV_INVALID_ARGUMENT;
  }
}

// One entry of the expression table where an operand names it (`ex`: the node, the operand and the expression; the message adds the token).
int check_expr(const llkv_having_expr &e, const std::string &ex, uint32_t n_keys, uint32_t n_aggs, std::string *err) {
  if (e.n_tokens == 0 || !e.tokens) { *err = ex + " is empty: no value is left"; return LLKV_INVALID_ARGUMENT; }
  uint64_t depth = 0;
  for (uint32_t t = 0; t < e.n_tokens; ++t) {
    const llkv_having_token &tk = e.tokens[t];
    const std::string where = ex + " token " + std::to_string(t) + " (" + token_name(tk.op) + ")";
    uint64_t pops = 0;
    switch (tk.op) {
    case LLKV_HAVING_TOKEN_PUSH:
      if (tk.leaf.kind == LLKV_HAVING_OPERAND_EXPR) { *err = where + ": the leaf is an expression (a leaf is a key, an aggregate or a literal)"; return LLKV_INVALID_ARGUMENT; }
      if (int rc = check_operand(tk.leaf, n_keys, n_aggs, ExprTable{nullptr, 0}, where + " leaf", err)) return rc;
      break;
    case LLKV_HAVING_TOKEN_ADD: case LLKV_HAVING_TOKEN_SUB: case LLKV_HAVING_TOKEN_MUL: case LLKV_HAVING_TOKEN_DIV: case LLKV_HAVING_TOKEN_MOD:
    case LLKV_HAVING_TOKEN_SHL: case LLKV_HAVING_TOKEN_SHR: pops = 2; break;
    case LLKV_HAVING_TOKEN_CAST_INT: case LLKV_HAVING_TOKEN_CAST_FLOAT: pops = 1; break;
    case LLKV_HAVING_TOKEN_COALESCE:
      if (tk.arg == 0) { *err = where + ": arg = 0"; return LLKV_INVALID_ARGUMENT; }
      pops = tk.arg;
      break;
    default: *err = ex + " token " + std::to_string(t) + ": unknown op " + std::to_string(tk.op); return LLKV_INVALID_ARGUMENT;
    }
    if (pops > depth) { *err = where + ": value stack underflow (pops " + std::to_string(pops) + " of " + std::to_string(depth) + " values)"; return LLKV_INVALID_ARGUMENT; }
    depth = depth - pops + 1;
    if (depth > kHavingMaxValueDepth) { *err = where + ": more than " + std::to_string(kHavingMaxValueDepth) + " pending values"; return LLKV_INVALID_ARGUMENT; }
  }
  if (depth != 1) {
    *err = ex + " token " + std::to_string(e.n_tokens - 1) + " (" + token_name(e.tokens[e.n_tokens - 1].op) + "): " + std::to_string(depth) + " values are left, not one";
    return LLKV_INVALID_ARGUMENT;
  }
  return LLKV_OK;
}

} // namespace

void HavingProgram::assign(const llkv_having_node *src, uint32_t n, const llkv_having_expr *ex, uint32_t n_ex) {
  nodes.assign(src, src + n);
  lists.clear();
  strings.clear();
  exprs.clear();
  tokens.clear();
  if (n) // (leaves inside expressions are never strings: set_having_ex refuses them)
    for (uint32_t x = 0; x < n_ex; ++x) {
      const uint32_t nt = ex[x].tokens ? ex[x].n_tokens : 0; // (an entry no operand names went unchecked)
      tokens.emplace_back(ex[x].tokens, ex[x].tokens + nt);
      exprs.push_back({tokens.back().data(), nt});
    }
  auto own = [&](llkv_having_operand &o) {
    if (o.kind != LLKV_HAVING_OPERAND_LITERAL || o.literal.tag != LLKV_LIT_STRING) return;
    strings.emplace_back(o.literal.str ? o.literal.str : "");
    o.literal.str = strings.back().c_str();
  };
  for (llkv_having_node &nd : nodes) {
    own(nd.lhs);
    own(nd.rhs);
    if (nd.kind != LLKV_HAVING_IN_LIST || nd.n_list == 0) { nd.list = nullptr; nd.n_list = 0; continue; }
    lists.emplace_back(nd.list, nd.list + nd.n_list);
    for (llkv_having_operand &o : lists.back()) own(o);
    nd.list = lists.back().data();
  }
}

int having_validate(const llkv_having_node *nodes, uint32_t n, const llkv_having_expr *exprs, uint32_t n_exprs, uint32_t n_keys, uint32_t n_aggs, std::string *err) {
  if (n == 0 || !nodes) { *err = "HAVING program is empty: no value is left"; return LLKV_INVALID_ARGUMENT; }
  if (n_exprs && !exprs) { *err = "HAVING expression table is NULL"; return LLKV_INVALID_ARGUMENT; }
  const ExprTable x{exprs, n_exprs}; // an expression is checked where an operand names it
  uint64_t depth = 0;
  int rc;
  for (uint32_t i = 0; i < n; ++i) {
    const llkv_having_node &nd = nodes[i];
    const std::string where = node_name(i, nd.kind);
    uint64_t pops = 0;
    switch (nd.kind) {
    case LLKV_HAVING_COMPARE:
      if (nd.cmp_op < LLKV_CMP_EQ || nd.cmp_op > LLKV_CMP_GT_EQ) { *err = where + ": unknown compare operator " + std::to_string(nd.cmp_op); return LLKV_INVALID_ARGUMENT; }
      if ((rc = check_operand(nd.lhs, n_keys, n_aggs, x, where + " lhs", err)) || (rc = check_operand(nd.rhs, n_keys, n_aggs, x, where + " rhs", err))) return rc;
      break;
    case LLKV_HAVING_IN_LIST:
      if ((rc = check_operand(nd.lhs, n_keys, n_aggs, x, where + " lhs", err))) return rc;
      if (nd.n_list && !nd.list) { *err = where + ": list is NULL"; return LLKV_INVALID_ARGUMENT; }
      for (uint32_t j = 0; j < nd.n_list; ++j)
        if ((rc = check_operand(nd.list[j], n_keys, n_aggs, x, where + " list item " + std::to_string(j), err))) return rc;
      break;
    case LLKV_HAVING_IS_NULL:
      if ((rc = check_operand(nd.lhs, n_keys, n_aggs, x, where + " lhs", err))) return rc;
      break;
    case LLKV_HAVING_LITERAL: break;
    case LLKV_HAVING_AND: case LLKV_HAVING_OR:
      if (nd.n_children == 0) { *err = where + ": n_children = 0"; return LLKV_INVALID_ARGUMENT; }
      pops = nd.n_children;
      break;
    case LLKV_HAVING_NOT: pops = 1; break;
    default: *err = "HAVING node " + std::to_string(i) + ": unknown kind " + std::to_string(nd.kind); return LLKV_INVALID_ARGUMENT;
    }
    if (pops > depth) { *err = where + ": stack underflow (pops " + std::to_string(pops) + " of " + std::to_string(depth) + " values)"; return LLKV_INVALID_ARGUMENT; }
    depth = depth - pops + 1;
    if (depth > kHavingMaxDepth) { *err = where + ": more than " + std::to_string(kHavingMaxDepth) + " pending values"; return LLKV_INVALID_ARGUMENT; }
  }
  if (depth != 1) { *err = node_name(n - 1, nodes[n - 1].kind) + ": " + std::to_string(depth) + " values are left, not one"; return LLKV_INVALID_ARGUMENT; }
  return LLKV_OK;
}

// A validated program (having_validate) over one row of cells.
int having_eval(const llkv_having_node *nodes, uint32_t n, const llkv_having_expr *exprs, uint32_t n_exprs, const HavingCell &cell, int32_t *truth) {
  const ExprTable x{exprs, n_exprs};
  HavingStack st;
  int rc;
  for (uint32_t i = 0; i < n; ++i) {
    const llkv_having_node &nd = nodes[i];
    HavingValue l, r;
    const char *ls, *rs;
    switch (nd.kind) {
    case LLKV_HAVING_COMPARE:
      if ((rc = operand_value(nd.lhs, x, cell, &l, &ls)) || (rc = operand_value(nd.rhs, x, cell, &r, &rs))) return rc;
      st.push(having_compare(nd.cmp_op, l, r));
      break;
    case LLKV_HAVING_IN_LIST: {
      if ((rc = operand_value(nd.lhs, x, cell, &l, &ls))) return rc;
      if (l.tag == kHvNull) { st.push(kHavingNull); break; }
      bool found = false, has_null = false;
      for (uint32_t j = 0; j < nd.n_list && !found; ++j) {
        if ((rc = operand_value(nd.list[j], x, cell, &r, &rs))) return rc;
        if (r.tag == kHvNull) { has_null = true; continue; }
        found = (l.tag == kHvString && r.tag == kHvString) ? std::strcmp(ls, rs) == 0 : having_in_match(l, r);
      }
      st.push(having_in_result(found, has_null, nd.negated != 0));
      break;
    }
    case LLKV_HAVING_IS_NULL:
      if ((rc = operand_value(nd.lhs, x, cell, &l, &ls))) return rc;
      st.push((l.tag == kHvNull) != (nd.negated != 0) ? kHavingTrue : kHavingFalse);
      break;
    case LLKV_HAVING_LITERAL: st.push(nd.literal ? kHavingTrue : kHavingFalse); break;
    case LLKV_HAVING_AND: st.push(st.pop_and(nd.n_children)); break;
    case LLKV_HAVING_OR: st.push(st.pop_or(nd.n_children)); break;
    default: st.push(having_not(st.pop())); break; // NOT
    }
  }
  *truth = st.pop();
  return LLKV_OK;
}

} // namespace llkv

using namespace llkv;

extern "C" llkv_status llkv_hip_having_eval_ex(const llkv_having_node *nodes, uint32_t n_nodes, const llkv_having_expr *exprs, uint32_t n_exprs,
                                               const llkv_value *key_cells, const int32_t *key_dtypes, uint32_t n_keys, const llkv_value *agg_cells,
                                               uint32_t n_aggs, int32_t *truth) {
  if (!truth || (n_keys && (!key_cells || !key_dtypes)) || (n_aggs && !agg_cells)) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "NULL argument");
  std::string err;
  if (int rc = having_validate(nodes, n_nodes, exprs, n_exprs, n_keys, n_aggs, &err)) return (llkv_status)set_error(rc, err);
  return (llkv_status)having_eval(nodes, n_nodes, exprs, n_exprs, [&](const llkv_having_operand &o, llkv_value *v, int32_t *key_dtype) {
    if (o.kind == LLKV_HAVING_OPERAND_KEY) { *v = key_cells[o.index]; *key_dtype = key_dtypes[o.index]; }
    else *v = agg_cells[o.index];
    return (int)LLKV_OK;
  }, truth);
}

extern "C" llkv_status llkv_hip_having_eval(const llkv_having_node *nodes, uint32_t n_nodes, const llkv_value *key_cells, const int32_t *key_dtypes,
                                            uint32_t n_keys, const llkv_value *agg_cells, uint32_t n_aggs, int32_t *truth) {
  return llkv_hip_having_eval_ex(nodes, n_nodes, nullptr, 0, key_cells, key_dtypes, n_keys, agg_cells, n_aggs, truth);
}
