// planvalue_expr.cpp — see planvalue_expr.hpp.
#include "planvalue_expr.hpp"

#include "having_rules.h"

#include <cstring>

namespace llkv {

namespace {

const char *kind_name(int32_t kind) {
  switch (kind) {
  case LLKV_TOK_COLUMN: return "COLUMN";
  case LLKV_TOK_LITERAL: return "LITERAL";
  case LLKV_TOK_BINARY: return "BINARY";
  case LLKV_TOK_COMPARE: return "COMPARE";
  case LLKV_TOK_NOT: return "NOT";
  case LLKV_TOK_IS_NULL: return "IS_NULL";
  case LLKV_TOK_CAST: return "CAST";
  case LLKV_TOK_COALESCE: return "COALESCE";
  case LLKV_TOK_CASE: return "CASE";
  default: return "?";
  }
}
const char *class_name(int cls) {
  switch (cls) {
  case kPvNull: return "NULL";
  case kPvInteger: return "Integer";
  case kPvFloat: return "Float";
  case kPvString: return "String";
  case kPvDate32: return "Date32";
  default: return "Decimal";
  }
}
int refuse(std::string *err, int code, uint32_t i, int32_t kind, const std::string &what) {
  if (err) *err = "aggregate argument token " + std::to_string(i) + " (" + kind_name(kind) + "): " + what;
  return code;
}
bool numeric_or_null(const CondNode &v) { return v.cls == kPvInteger || v.cls == kPvFloat || v.cls == kPvNull; }

// COMPARE's admission of a pair (a simple CASE's operand / candidate pairs come here too): a Utf8 COLUMN compares against a
// String literal only — on the device it is a code mask over its dictionary
int check_compare_pair(const CondNode &l, const CondNode &r, uint32_t i, int32_t kind, std::string *err) {
  const auto str_col = [](const CondNode &v) { return v.cls == kPvString && v.origin == kCondColumn; };
  const auto str_lit = [](const CondNode &v) { return v.cls == kPvString && v.origin == kCondLiteral; };
  if ((str_col(l) && !str_lit(r)) || (str_col(r) && !str_lit(l)))
    return refuse(err, LLKV_UNSUPPORTED, i, kind, "a Utf8 column compares against a String literal only");
  return LLKV_OK;
}

// The value branches of a CASE / the items of a COALESCE: all Integer or all Float, NULL literals beside them — the group's temp
// column is typed by its first non-NULL value, and a later value of the other class is an error in the reference.
int branch_class(const std::vector<CondNode> &branches, uint32_t i, int32_t kind, int *cls, std::string *err) {
  int c = kPvNull;
  for (const CondNode &b : branches) {
    if (b.cls == kPvNull) continue;
    if (b.cls != kPvInteger && b.cls != kPvFloat)
      return refuse(err, LLKV_UNSUPPORTED, i, kind, std::string("a ") + class_name(b.cls) + " value branch (String and Date32 values are served as COMPARE sides and under IS NULL only)");
    if (c != kPvNull && c != b.cls)
      return refuse(err, LLKV_UNSUPPORTED, i, kind, "value branches of mixed classes (Integer and Float): the result type would depend on the data — write the branches in one class, e.g. ELSE 0.0");
    c = b.cls;
  }
  if (c == kPvNull) return refuse(err, LLKV_UNSUPPORTED, i, kind, "only NULL value branches");
  *cls = c;
  return LLKV_OK;
}

} // namespace

bool cond_program(const llkv_expr_token *e, uint32_t n) {
  for (uint32_t i = 0; e && i < n; ++i) {
    if (e[i].kind != LLKV_TOK_COLUMN && e[i].kind != LLKV_TOK_LITERAL && e[i].kind != LLKV_TOK_BINARY) return true;
    if (e[i].kind == LLKV_TOK_BINARY && (e[i].binop == LLKV_BIN_AND || e[i].binop == LLKV_BIN_OR)) return true;
  }
  return false;
}

int cond_refuse_elsewhere(const llkv_expr_token *e, uint32_t n, const char *where, std::string *err) {
  for (uint32_t i = 0; e && i < n; ++i) {
    const bool logic = e[i].kind == LLKV_TOK_BINARY && (e[i].binop == LLKV_BIN_AND || e[i].binop == LLKV_BIN_OR);
    if (e[i].kind == LLKV_TOK_COLUMN || e[i].kind == LLKV_TOK_LITERAL || (e[i].kind == LLKV_TOK_BINARY && !logic)) continue;
    if (e[i].kind < LLKV_TOK_COLUMN || e[i].kind > LLKV_TOK_CASE) {
      if (err) *err = std::string(where) + ": token " + std::to_string(i) + ": unknown token kind " + std::to_string(e[i].kind);
      return LLKV_INVALID_ARGUMENT;
    }
    if (err) *err = std::string(where) + ": token " + std::to_string(i) + " (" + (logic ? (e[i].binop == LLKV_BIN_AND ? "AND" : "OR") : kind_name(e[i].kind)) +
                    "): conditional expressions are served in GROUP BY aggregate arguments only";
    return LLKV_UNSUPPORTED;
  }
  return LLKV_OK;
}

int cond_class_of_dtype(int32_t dtype) {
  switch (dtype) {
  case LLKV_DT_INT64: case LLKV_DT_INT32: case LLKV_DT_UINT32: return kPvInteger;
  case LLKV_DT_FLOAT64: case LLKV_DT_FLOAT32: return kPvFloat;
  case LLKV_DT_UTF8: return kPvString;
  case LLKV_DT_DATE32: return kPvDate32;
  case LLKV_DT_DECIMAL128: return kPvDecimal;
  default: return -1;
  }
}

int cond_static_check(const llkv_expr_token *e, uint32_t n, const CondLeafClass &leaf, std::vector<CondNode> *nodes, std::string *err) {
  std::vector<CondNode> st;
  nodes->assign(n, CondNode{});
  if (!e || n == 0) { if (err) *err = "aggregate requires an argument"; return LLKV_INVALID_ARGUMENT; }
  if (n > kCondMaxTokens) { if (err) *err = "aggregate argument of " + std::to_string(n) + " tokens: more than " + std::to_string(kCondMaxTokens); return LLKV_UNSUPPORTED; }
  for (uint32_t i = 0; i < n; ++i) {
    const llkv_expr_token &t = e[i];
    const auto need = [&](size_t k) { return st.size() >= k ? LLKV_OK : refuse(err, LLKV_INVALID_ARGUMENT, i, t.kind, "stack underflow (" + std::to_string(k) + " operands wanted, " + std::to_string(st.size()) + " pending)"); };
    CondNode out;
    int rc;
    switch (t.kind) {
    case LLKV_TOK_COLUMN: {
      const int cls = leaf(t.field_id);
      if (cls == -2) { if (err) *err = "field " + std::to_string(t.field_id) + " not found"; return LLKV_NOT_FOUND; }
      if (cls == kPvDecimal) return refuse(err, LLKV_UNSUPPORTED, i, t.kind, "a Decimal128 column in a conditional expression");
      if (cls < 0) return refuse(err, LLKV_UNSUPPORTED, i, t.kind, "a column of this type in a conditional expression");
      out = {cls, kCondColumn};
      break;
    }
    case LLKV_TOK_LITERAL:
      switch (t.literal.tag) {
      case LLKV_LIT_NULL: out = {kPvNull, kCondLiteral}; break;
      case LLKV_LIT_INT128: case LLKV_LIT_BOOLEAN: out = {kPvInteger, kCondLiteral}; break;
      case LLKV_LIT_FLOAT64: out = {kPvFloat, kCondLiteral}; break;
      case LLKV_LIT_STRING:
        if (!t.literal.str) return refuse(err, LLKV_INVALID_ARGUMENT, i, t.kind, "a String literal without a string");
        out = {kPvString, kCondLiteral};
        break;
      case LLKV_LIT_DATE32: out = {kPvDate32, kCondLiteral}; break;
      case LLKV_LIT_DECIMAL128: return refuse(err, LLKV_UNSUPPORTED, i, t.kind, "a Decimal128 literal in a conditional expression");
      default: return refuse(err, LLKV_INVALID_ARGUMENT, i, t.kind, "unknown literal tag " + std::to_string(t.literal.tag));
      }
      break;
    case LLKV_TOK_BINARY: {
      if (t.binop < LLKV_BIN_ADD || t.binop > LLKV_BIN_OR) return refuse(err, LLKV_INVALID_ARGUMENT, i, t.kind, "unknown binary op " + std::to_string(t.binop));
      if ((rc = need(2))) return rc;
      const CondNode r = st.back(); st.pop_back();
      const CondNode l = st.back(); st.pop_back();
      if (!numeric_or_null(l) || !numeric_or_null(r))
        return refuse(err, LLKV_UNSUPPORTED, i, t.kind, std::string("a ") + class_name(numeric_or_null(l) ? r.cls : l.cls) + " operand (String and Date32 values are served as COMPARE sides and under IS NULL only)");
      const bool logic = t.binop == LLKV_BIN_AND || t.binop == LLKV_BIN_OR;
      out.cls = (!logic && (l.cls == kPvFloat || r.cls == kPvFloat)) ? kPvFloat : kPvInteger;
      break;
    }
    case LLKV_TOK_COMPARE: {
      if (t.binop < LLKV_CMP_EQ || t.binop > LLKV_CMP_GT_EQ) return refuse(err, LLKV_INVALID_ARGUMENT, i, t.kind, "unknown compare op " + std::to_string(t.binop));
      if ((rc = need(2))) return rc;
      const CondNode r = st.back(); st.pop_back();
      const CondNode l = st.back(); st.pop_back();
      if ((rc = check_compare_pair(l, r, i, t.kind, err))) return rc;
      out.cls = kPvInteger;
      break;
    }
    case LLKV_TOK_NOT: {
      if ((rc = need(1))) return rc;
      const CondNode v = st.back(); st.pop_back();
      if (!numeric_or_null(v)) return refuse(err, LLKV_UNSUPPORTED, i, t.kind, std::string("a ") + class_name(v.cls) + " operand (an error in the reference)");
      out.cls = kPvInteger;
      break;
    }
    case LLKV_TOK_IS_NULL:
      if ((rc = need(1))) return rc;
      st.pop_back();
      out.cls = kPvInteger;
      break;
    case LLKV_TOK_CAST: {
      if ((rc = need(1))) return rc;
      const CondNode v = st.back(); st.pop_back();
      if (t.binop == LLKV_DT_INT64 || t.binop == LLKV_DT_INT32) out.cls = kPvInteger;
      else if (t.binop == LLKV_DT_FLOAT64 || t.binop == LLKV_DT_FLOAT32) out.cls = kPvFloat;
      else return refuse(err, LLKV_UNSUPPORTED, i, t.kind, "target dtype " + std::to_string(t.binop) + " (Int64 / Int32 / Float64 / Float32 are served)");
      if (!numeric_or_null(v)) return refuse(err, LLKV_UNSUPPORTED, i, t.kind, std::string("a ") + class_name(v.cls) + " source");
      break;
    }
    case LLKV_TOK_COALESCE: {
      const uint32_t k = t.field_id;
      if (k == 0) return refuse(err, LLKV_INVALID_ARGUMENT, i, t.kind, "no items");
      if (k > kCondMaxItems) return refuse(err, LLKV_UNSUPPORTED, i, t.kind, std::to_string(k) + " items: more than " + std::to_string(kCondMaxItems));
      if ((rc = need(k))) return rc;
      const std::vector<CondNode> items(st.end() - k, st.end());
      st.resize(st.size() - k);
      if ((rc = branch_class(items, i, t.kind, &out.cls, err))) return rc;
      break;
    }
    case LLKV_TOK_CASE: {
      const uint32_t w = t.field_id;
      if (w == 0) return refuse(err, LLKV_INVALID_ARGUMENT, i, t.kind, "no WHEN / THEN pair");
      if (t.binop & ~(LLKV_CASE_HAS_OPERAND | LLKV_CASE_HAS_ELSE)) return refuse(err, LLKV_INVALID_ARGUMENT, i, t.kind, "unknown flags " + std::to_string(t.binop));
      if (w > kCondMaxWhens) return refuse(err, LLKV_UNSUPPORTED, i, t.kind, std::to_string(w) + " WHEN / THEN pairs: more than " + std::to_string(kCondMaxWhens));
      const bool simple = t.binop & LLKV_CASE_HAS_OPERAND, has_else = t.binop & LLKV_CASE_HAS_ELSE;
      const size_t total = (simple ? 1 : 0) + 2 * (size_t)w + (has_else ? 1 : 0);
      if ((rc = need(total))) return rc;
      const std::vector<CondNode> a(st.end() - total, st.end());
      st.resize(st.size() - total);
      std::vector<CondNode> branches;
      if (simple && a[0].cls == kPvDate32) return refuse(err, LLKV_UNSUPPORTED, i, t.kind, "a Date32 operand of a simple CASE");
      for (uint32_t k = 0; k < w; ++k) {
        const CondNode &when = a[(simple ? 1 : 0) + 2 * k];
        if (simple) {
          if (when.cls == kPvDate32) return refuse(err, LLKV_UNSUPPORTED, i, t.kind, "a Date32 candidate of a simple CASE");
          if ((rc = check_compare_pair(a[0], when, i, t.kind, err))) return rc;
        } else if (!numeric_or_null(when))
          return refuse(err, LLKV_UNSUPPORTED, i, t.kind, std::string("a ") + class_name(when.cls) + " WHEN (String and Date32 values are served as COMPARE sides and under IS NULL only)");
        branches.push_back(a[(simple ? 1 : 0) + 2 * k + 1]);
      }
      if (has_else) branches.push_back(a.back());
      if ((rc = branch_class(branches, i, t.kind, &out.cls, err))) return rc;
      break;
    }
    default: return refuse(err, LLKV_INVALID_ARGUMENT, i, t.kind, "unknown token kind " + std::to_string(t.kind));
    }
    (*nodes)[i] = out;
    st.push_back(out);
  }
  if (st.size() != 1) return refuse(err, LLKV_INVALID_ARGUMENT, n - 1, e[n - 1].kind, std::to_string(st.size()) + " values left on the stack");
  if (st[0].cls != kPvInteger && st[0].cls != kPvFloat)
    return refuse(err, LLKV_UNSUPPORTED, n - 1, e[n - 1].kind, std::string("a ") + class_name(st[0].cls) + " value as the aggregate's argument");
  return LLKV_OK;
}

// ---- one row -------------------------------------------------------------------------------------------------------------------
namespace {

struct RowValue { // CondValue plus the classes only COMPARE and IS NULL look at
  int cls = kPvNull;
  int64_t i = 0;
  double f = 0.0;
  std::string s;
};
RowValue integer(int64_t v) { RowValue r; r.cls = kPvInteger; r.i = v; return r; }
RowValue flt(double v) { RowValue r; r.cls = kPvFloat; r.f = v; return r; }
bool truth(const RowValue &v) { return v.cls == kPvInteger ? pv_truth(v.i) : v.cls == kPvFloat ? pv_truth(v.f) : false; }

RowValue compare(int op, const RowValue &l, const RowValue &r) {
  if (l.cls == kPvNull || r.cls == kPvNull) return RowValue{};
  if (!pv_comparable(l.cls, r.cls)) return integer(0);
  if (l.cls == kPvString) {
    const int c = l.s.compare(r.s); // bytes, then lengths (char_traits<char>::compare is memcmp)
    return integer(pv_compare_bytes(op, (c > 0) - (c < 0)) ? 1 : 0);
  }
  bool m;
  if (l.cls == kPvInteger && r.cls == kPvInteger) m = pv_compare(op, l.i, r.i);
  else if (l.cls == kPvInteger) m = pv_compare(op, l.i, r.f);
  else if (r.cls == kPvInteger) m = pv_compare(op, l.f, r.i);
  else m = pv_compare(op, l.f, r.f);
  return integer(m ? 1 : 0);
}

// + − * / % of the PlanValue interpreter (:7193-7389): having_rules.h holds the one copy (its ops: 2 ADD … 6 MOD)
RowValue arith(int binop, const RowValue &l, const RowValue &r) {
  const auto hv = [](const RowValue &v) {
    HavingValue h{v.cls == kPvInteger ? kHvInteger : v.cls == kPvFloat ? kHvFloat : kHvNull, 0};
    if (v.cls == kPvInteger) h.bits = (uint64_t)v.i;
    else if (v.cls == kPvFloat) std::memcpy(&h.bits, &v.f, 8);
    return h;
  };
  const HavingValue o = having_arith(binop + 1, hv(l), hv(r));
  if (o.tag == kHvInteger) return integer((int64_t)o.bits);
  if (o.tag == kHvFloat) { double d; std::memcpy(&d, &o.bits, 8); return flt(d); }
  return RowValue{};
}

} // namespace

int cond_eval_row(const llkv_expr_token *e, uint32_t n, const CondCellOf &cell, CondValue *out, std::string *err) {
  std::vector<CondNode> nodes;
  const CondLeafClass leaf = [&](uint32_t field) { const CondCell *c = cell(field); return c ? c->cls : -2; };
  if (int rc = cond_static_check(e, n, leaf, &nodes, err)) return rc;
  std::vector<RowValue> st;
  for (uint32_t i = 0; i < n; ++i) {
    const llkv_expr_token &t = e[i];
    RowValue o;
    switch (t.kind) {
    case LLKV_TOK_COLUMN: {
      const CondCell &c = *cell(t.field_id);
      if (!c.is_null) { o.cls = c.cls; o.i = c.i; o.f = c.f; o.s = c.s; }
      break;
    }
    case LLKV_TOK_LITERAL:
      o.cls = nodes[i].cls;
      if (t.literal.tag == LLKV_LIT_INT128 || t.literal.tag == LLKV_LIT_DATE32) o.i = (int64_t)t.literal.lo; // `*v as i64`
      else if (t.literal.tag == LLKV_LIT_BOOLEAN) o.i = t.literal.lo ? 1 : 0;
      else if (t.literal.tag == LLKV_LIT_FLOAT64) o.f = t.literal.f64;
      else if (t.literal.tag == LLKV_LIT_STRING) o.s = t.literal.str;
      break;
    case LLKV_TOK_BINARY: {
      const RowValue r = st.back(); st.pop_back();
      const RowValue l = st.back(); st.pop_back();
      if (t.binop == LLKV_BIN_AND || t.binop == LLKV_BIN_OR) {
        bool known;
        const bool v = t.binop == LLKV_BIN_AND ? pv_and(truth(l), l.cls != kPvNull, truth(r), r.cls != kPvNull, &known)
                                               : pv_or(truth(l), l.cls != kPvNull, truth(r), r.cls != kPvNull, &known);
        if (known) o = integer(v ? 1 : 0);
      } else o = arith(t.binop, l, r);
      break;
    }
    case LLKV_TOK_COMPARE: {
      const RowValue r = st.back(); st.pop_back();
      const RowValue l = st.back(); st.pop_back();
      o = compare(t.binop, l, r);
      break;
    }
    case LLKV_TOK_NOT: {
      const RowValue v = st.back(); st.pop_back();
      if (v.cls != kPvNull) o = integer(pv_not(truth(v)));
      break;
    }
    case LLKV_TOK_IS_NULL: {
      const RowValue v = st.back(); st.pop_back();
      o = integer(((v.cls == kPvNull) != (t.binop != 0)) ? 1 : 0);
      break;
    }
    case LLKV_TOK_CAST: {
      const RowValue v = st.back(); st.pop_back();
      if (v.cls == kPvNull) break;
      if (nodes[i].cls == kPvInteger) o = integer(v.cls == kPvInteger ? pv_cast_i64(v.i) : pv_cast_i64(v.f));
      else o = flt(v.cls == kPvInteger ? pv_cast_f64(v.i) : pv_cast_f64(v.f));
      break;
    }
    case LLKV_TOK_COALESCE: {
      const uint32_t k = t.field_id;
      for (size_t j = st.size() - k; j < st.size(); ++j) if (st[j].cls != kPvNull) { o = st[j]; break; }
      st.resize(st.size() - k);
      break;
    }
    default: { // LLKV_TOK_CASE
      const uint32_t w = t.field_id;
      const bool simple = t.binop & LLKV_CASE_HAS_OPERAND, has_else = t.binop & LLKV_CASE_HAS_ELSE;
      const size_t total = (simple ? 1 : 0) + 2 * (size_t)w + (has_else ? 1 : 0), at = st.size() - total;
      if (has_else) o = st.back();
      for (uint32_t k = w; k-- > 0;) { // last pair first: the first true branch is the one written last
        const RowValue &when = st[at + (simple ? 1 : 0) + 2 * k];
        const bool hit = simple ? truth(compare(LLKV_CMP_EQ, st[at], when)) : truth(when);
        if (hit) o = st[at + (simple ? 1 : 0) + 2 * k + 1];
      }
      st.resize(at);
      break;
    }
    }
    st.push_back(o);
  }
  out->cls = st[0].cls;
  out->i = st[0].i;
  out->f = st[0].f;
  return LLKV_OK;
}

} // namespace llkv
