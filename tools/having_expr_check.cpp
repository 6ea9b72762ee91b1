// having_expr_check.cpp — a stand-alone host program (no GPU, no Python) that feeds the edge table of HAVING value expressions
// through llkv_hip_having_eval_ex: csrc/having.cpp and csrc/having_rules.h alone, so that the host sanitizers can watch them.
// tools/sanitize_having.sh builds it with -fsanitize=address,undefined and runs it.
// (hipcc only for the HIP headers engine.hpp includes; nothing is compiled for a device.)  Exit status 0: every row matched.
#include "engine.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace llkv { // what having.cpp takes from engine.cpp
thread_local std::string g_last_error;
int set_error(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}
} // namespace llkv

namespace {

struct Cell {
  char type; // 'n' NULL, 'i' Int64, 'f' Float64
  int64_t i;
  double f;
};
Cell N() { return {'n', 0, 0}; }
Cell I(int64_t v) { return {'i', v, 0}; }
Cell F(double v) { return {'f', 0, v}; }

llkv_value to_value(const Cell &c) {
  llkv_value v;
  std::memset(&v, 0, sizeof v);
  v.dtype = c.type == 'f' ? LLKV_DT_FLOAT64 : LLKV_DT_INT64;
  v.is_null = c.type == 'n';
  v.i64 = c.i;
  v.f64 = c.f;
  return v;
}

llkv_having_operand agg(uint32_t index) {
  llkv_having_operand o;
  std::memset(&o, 0, sizeof o);
  o.kind = LLKV_HAVING_OPERAND_AGGREGATE;
  o.index = index;
  return o;
}
llkv_having_operand lit(const Cell &c) {
  llkv_having_operand o;
  std::memset(&o, 0, sizeof o);
  o.kind = LLKV_HAVING_OPERAND_LITERAL;
  o.literal.tag = c.type == 'n' ? LLKV_LIT_NULL : c.type == 'i' ? LLKV_LIT_INT128 : LLKV_LIT_FLOAT64;
  o.literal.lo = (uint64_t)c.i;
  o.literal.hi = c.i < 0 ? -1 : 0;
  o.literal.f64 = c.f;
  return o;
}
llkv_having_operand expr(uint32_t index) {
  llkv_having_operand o;
  std::memset(&o, 0, sizeof o);
  o.kind = LLKV_HAVING_OPERAND_EXPR;
  o.index = index;
  return o;
}
llkv_having_token push(const llkv_having_operand &leaf) { return {LLKV_HAVING_TOKEN_PUSH, 0, leaf}; }
llkv_having_token tok(int32_t op, uint32_t arg = 0) {
  llkv_having_token t;
  std::memset(&t, 0, sizeof t);
  t.op = op;
  t.arg = arg;
  return t;
}

int failures = 0;

// truth of one node over the expression `tokens` and the cells
int truth_of(const llkv_having_node &node, const std::vector<llkv_having_token> &tokens, const std::vector<Cell> &cells) {
  std::vector<llkv_value> aggs;
  for (const Cell &c : cells) aggs.push_back(to_value(c));
  const llkv_having_expr e{tokens.data(), (uint32_t)tokens.size()};
  int32_t truth = 99;
  const llkv_status rc = llkv_hip_having_eval_ex(&node, 1, &e, 1, nullptr, nullptr, 0, aggs.data(), (uint32_t)aggs.size(), &truth);
  if (rc != LLKV_OK) {
    std::printf("  status %d: %s\n", (int)rc, llkv::g_last_error.c_str());
    return 98;
  }
  return truth;
}

// The expression's value is `want`: IS NULL says whether it is Null; an Integer equals the Integer literal and neither neighbour;
// a Float equals the Float literal (NaN: != itself), and CAST_INT of it differs from it unless it is integral.
void expect(const char *what, std::vector<llkv_having_token> tokens, const std::vector<Cell> &cells, const Cell &want) {
  llkv_having_node n;
  std::memset(&n, 0, sizeof n);
  n.kind = LLKV_HAVING_IS_NULL;
  n.lhs = expr(0);
  bool ok = truth_of(n, tokens, cells) == (want.type == 'n' ? 1 : 0);
  n.kind = LLKV_HAVING_COMPARE;
  n.cmp_op = LLKV_CMP_EQ;
  n.rhs = lit(want);
  if (want.type == 'n') {
    n.rhs = lit(I(1));
    ok = ok && truth_of(n, tokens, cells) == -1; // the enclosing compare is NULL
  } else if (want.type == 'f' && std::isnan(want.f)) {
    ok = ok && truth_of(n, tokens, cells) == 0;
    n.cmp_op = LLKV_CMP_NOT_EQ;
    ok = ok && truth_of(n, tokens, cells) == 1;
  } else {
    ok = ok && truth_of(n, tokens, cells) == 1;
    if (want.type == 'i') {
      if (want.i > INT64_MIN) { n.rhs = lit(I(want.i - 1)); ok = ok && truth_of(n, tokens, cells) == 0; }
      if (want.i < INT64_MAX) { n.rhs = lit(I(want.i + 1)); ok = ok && truth_of(n, tokens, cells) == 0; }
    } else {
      // a Float: x / 2 * 2 (by the Integers 2) gives it back — an Integer 2^53 or beyond, or an odd one, would not
      tokens.push_back(push(lit(I(2))));
      tokens.push_back(tok(LLKV_HAVING_TOKEN_DIV));
      tokens.push_back(push(lit(I(2))));
      tokens.push_back(tok(LLKV_HAVING_TOKEN_MUL));
      n.rhs = lit(want);
      if (std::isfinite(want.f) && std::fabs(want.f) > 1e-300) ok = ok && truth_of(n, tokens, cells) == 1;
    }
  }
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
  if (!ok) ++failures;
}

std::vector<llkv_having_token> binary(int32_t op) { return {push(agg(0)), push(agg(1)), tok(op)}; }
std::vector<llkv_having_token> unary(int32_t op) { return {push(agg(0)), tok(op)}; }

} // namespace

int main() {
  const int64_t MIN = INT64_MIN, MAX = INT64_MAX;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const int32_t ADD = LLKV_HAVING_TOKEN_ADD, SUB = LLKV_HAVING_TOKEN_SUB, MUL = LLKV_HAVING_TOKEN_MUL, DIV = LLKV_HAVING_TOKEN_DIV, MOD = LLKV_HAVING_TOKEN_MOD,
                SHL = LLKV_HAVING_TOKEN_SHL, SHR = LLKV_HAVING_TOKEN_SHR;
  expect("i64::MIN / -1 = Float 2^63", binary(DIV), {I(MIN), I(-1)}, F(9.223372036854775808e18));
  expect("-7 / 2 = -3", binary(DIV), {I(-7), I(2)}, I(-3));
  expect("x / 0 is NULL", binary(DIV), {I(5), I(0)}, N());
  expect("x / 0.0 is NULL", binary(DIV), {I(5), F(0.0)}, N());
  expect("x / -0.0 is NULL", binary(DIV), {I(5), F(-0.0)}, N());
  expect("x % 0 is NULL", binary(MOD), {I(5), I(0)}, N());
  expect("-7 % 3 = -1", binary(MOD), {I(-7), I(3)}, I(-1));
  expect("5.5 % -2.0 = 1.5", binary(MOD), {F(5.5), F(-2.0)}, F(1.5));
  expect("(2^53 + 1) + 0 = 2^53", binary(ADD), {I((1ll << 53) + 1), I(0)}, I(1ll << 53));
  expect("(2^62 + 1) % 2 = 0", binary(MOD), {I((1ll << 62) + 1), I(2)}, I(0));
  expect("i64::MAX * 2 = i64::MAX", binary(MUL), {I(MAX), I(2)}, I(MAX));
  expect("i64::MIN - 1 = i64::MIN", binary(SUB), {I(MIN), I(1)}, I(MIN));
  expect("i64::MAX * i64::MIN = i64::MIN", binary(MUL), {I(MAX), I(MIN)}, I(MIN));
  expect("0.0 * inf is NaN", binary(MUL), {F(0.0), F(inf)}, F(nan));
  expect("inf % 2.0 is NaN", binary(MOD), {F(inf), F(2.0)}, F(nan));
  expect("7 / 2.0 = Float 3.5", binary(DIV), {I(7), F(2.0)}, F(3.5));
  expect("8.0 / 2 = Float 4.0", binary(DIV), {F(8.0), I(2)}, F(4.0));
  expect("2 + 3.5 = Float 5.5", binary(ADD), {I(2), F(3.5)}, F(5.5));
  expect("1 << 64 = 1", binary(SHL), {I(1), I(64)}, I(1));
  expect("1 << 65 = 2", binary(SHL), {I(1), I(65)}, I(2));
  expect("-8 >> 1 = -4", binary(SHR), {I(-8), I(1)}, I(-4));
  expect("1 << 63 = i64::MIN", binary(SHL), {I(1), I(63)}, I(MIN));
  expect("i64::MIN << 1 = 0", binary(SHL), {I(MIN), I(1)}, I(0));
  expect("3 << 2.9 = 12 (a Float count)", binary(SHL), {I(3), F(2.9)}, I(12));
  expect("1e30 >> 1 = i64::MAX >> 1", binary(SHR), {F(1e30), I(1)}, I(MAX >> 1));
  expect("7 << NaN = 7", binary(SHL), {I(7), F(nan)}, I(7));
  expect("NULL << 1 is NULL", binary(SHL), {N(), I(1)}, N());
  expect("CAST_INT(1e30) = i64::MAX", unary(LLKV_HAVING_TOKEN_CAST_INT), {F(1e30)}, I(MAX));
  expect("CAST_INT(-1e30) = i64::MIN", unary(LLKV_HAVING_TOKEN_CAST_INT), {F(-1e30)}, I(MIN));
  expect("CAST_INT(NaN) = 0", unary(LLKV_HAVING_TOKEN_CAST_INT), {F(nan)}, I(0));
  expect("CAST_INT(-2.9) = -2", unary(LLKV_HAVING_TOKEN_CAST_INT), {F(-2.9)}, I(-2));
  expect("CAST_FLOAT(2^53 + 1) = 2^53", unary(LLKV_HAVING_TOKEN_CAST_FLOAT), {I((1ll << 53) + 1)}, F(9007199254740992.0));
  expect("CAST_INT(NULL) is NULL", unary(LLKV_HAVING_TOKEN_CAST_INT), {N()}, N());
  expect("COALESCE(NULL, NULL) is NULL", {push(lit(N())), push(lit(N())), tok(LLKV_HAVING_TOKEN_COALESCE, 2)}, {}, N());
  expect("COALESCE(agg, 0) of a NULL aggregate = 0", {push(agg(0)), push(lit(I(0))), tok(LLKV_HAVING_TOKEN_COALESCE, 2)}, {N()}, I(0));
  expect("COALESCE(4, 2.5) = 4 (the first, not the last)", {push(agg(0)), push(agg(1)), tok(LLKV_HAVING_TOKEN_COALESCE, 2)}, {I(4), F(2.5)}, I(4));
  expect("COALESCE of eight (the deepest stack)",
         {push(lit(N())), push(lit(N())), push(lit(N())), push(lit(N())), push(lit(N())), push(lit(N())), push(lit(N())), push(lit(I(8))), tok(LLKV_HAVING_TOKEN_COALESCE, 8)},
         {}, I(8));
  expect("NULL + 1 is NULL", binary(ADD), {N(), I(1)}, N());
  expect("(a * a) - b rounds twice (no fma)", {push(agg(0)), push(agg(0)), tok(MUL), push(agg(1)), tok(SUB)},
         {F(1.0 + 0x1p-30), F((1.0 + 0x1p-30) * (1.0 + 0x1p-30))}, F(0.0));

  // the refusals own no memory either: a malformed expression and a non-numeric cell
  {
    llkv_having_node n;
    std::memset(&n, 0, sizeof n);
    n.kind = LLKV_HAVING_IS_NULL;
    n.lhs = expr(0);
    const bool a = truth_of(n, {push(agg(0)), tok(ADD)}, {I(1)}) == 98; // underflow
    const bool b = truth_of(n, {}, {I(1)}) == 98;                      // empty
    n.lhs = expr(3);
    const bool c = truth_of(n, {push(agg(0))}, {I(1)}) == 98; // index out of range
    std::printf("%s malformed expressions are refused\n", a && b && c ? "ok  " : "FAIL");
    if (!(a && b && c)) ++failures;
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
