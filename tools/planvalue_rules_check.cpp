// planvalue_rules_check.cpp — a stand-alone host program (no GPU, no Python) over csrc/planvalue_rules.h and csrc/planvalue_expr.cpp
// (the static check and the one-row evaluator of conditional GROUP BY aggregate arguments), so that the host sanitizers can watch
// them: an edge table of the rules, then every program of a small enumerated corpus — well-formed and malformed — over every row
// of an edge-cell table.  tools/sanitize_planvalue.sh builds it with -fsanitize=address,undefined and runs it.
//   g++ -std=c++17 -I include -I rust-llkv_amd/csrc tools/planvalue_rules_check.cpp rust-llkv_amd/csrc/planvalue_expr.cpp
// Exit status 0: every pinned row matched and nothing was flagged.
#include "planvalue_expr.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

using namespace llkv;

namespace {

int failures = 0;
void expect(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "MISMATCH: %s\n", what); ++failures; }
}

llkv_expr_token tok(int32_t kind, int32_t binop = 0, uint32_t field = 0) {
  llkv_expr_token t;
  std::memset(&t, 0, sizeof t);
  t.kind = kind; t.binop = binop; t.field_id = field;
  return t;
}
llkv_expr_token lit_i(int64_t v) { llkv_expr_token t = tok(LLKV_TOK_LITERAL); t.literal.tag = LLKV_LIT_INT128; t.literal.lo = (uint64_t)v; t.literal.hi = v < 0 ? -1 : 0; return t; }
llkv_expr_token lit_f(double v) { llkv_expr_token t = tok(LLKV_TOK_LITERAL); t.literal.tag = LLKV_LIT_FLOAT64; t.literal.f64 = v; return t; }
llkv_expr_token lit_s(const char *s) { llkv_expr_token t = tok(LLKV_TOK_LITERAL); t.literal.tag = LLKV_LIT_STRING; t.literal.str = s; return t; }
llkv_expr_token lit_null() { llkv_expr_token t = tok(LLKV_TOK_LITERAL); t.literal.tag = LLKV_LIT_NULL; return t; }
llkv_expr_token lit_date(int64_t d) { llkv_expr_token t = tok(LLKV_TOK_LITERAL); t.literal.tag = LLKV_LIT_DATE32; t.literal.lo = (uint64_t)d; return t; }
llkv_expr_token column(uint32_t f) { return tok(LLKV_TOK_COLUMN, 0, f); }

using Program = std::vector<llkv_expr_token>;
Program cat(std::initializer_list<Program> parts) { Program p; for (const Program &x : parts) p.insert(p.end(), x.begin(), x.end()); return p; }

struct Row { CondCell c[5]; }; // fields 1 Int, 2 Float, 3 String, 4 Date32, 5 Int
int eval(const Program &p, const Row &row, CondValue *v, std::string *err) {
  const CondCellOf cell = [&](uint32_t f) -> const CondCell * { return f >= 1 && f <= 5 ? &row.c[f - 1] : nullptr; };
  return cond_eval_row(p.data(), (uint32_t)p.size(), cell, v, err);
}

} // namespace

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  // ---- the rules header
  expect(pv_f64_as_i64(nan) == 0 && pv_f64_as_i64(inf) == INT64_MAX && pv_f64_as_i64(-inf) == INT64_MIN && pv_f64_as_i64(9.3e18) == INT64_MAX && pv_f64_as_i64(-2.9) == -2, "f64 as i64");
  for (int op = 1; op <= 6; ++op) {
    expect(pv_compare(op, nan, 1.0) == (op == 2) && pv_compare(op, nan, nan) == (op == 2), "a NaN operand: only != holds");
    expect(pv_compare(op, (int64_t)((1ll << 53) + 1), 9007199254740992.0) == (op == 1 || op == 4 || op == 6), "Integer against Float through f64");
    expect(pv_compare(op, (int64_t)((1ll << 53) + 1), (int64_t)(1ll << 53)) == (op == 2 || op == 5 || op == 6), "Int / Int natively");
    expect(pv_compare_bytes(op, -1) == (op == 2 || op == 3 || op == 4), "bytes");
  }
  expect(!pv_rel<int64_t>(0, 1, 1) && !pv_comparable(kPvDate32, kPvDate32) && !pv_comparable(kPvInteger, kPvString) && pv_comparable(kPvInteger, kPvFloat) && pv_comparable(kPvString, kPvString), "pairings");
  expect(pv_truth(nan) && !pv_truth(-0.0) && pv_truth((int64_t)-1) && pv_not(true) == 0 && pv_not(false) == 1, "truth");
  for (int l = 0; l < 3; ++l) for (int r = 0; r < 3; ++r) { // 0 false, 1 true, 2 unknown
    bool k;
    const bool a = pv_and(l == 1, l != 2, r == 1, r != 2, &k);
    expect((l == 0 || r == 0) ? (k && !a) : (l == 2 || r == 2) ? !k : (k && a), "three-valued AND");
    const bool o = pv_or(l == 1, l != 2, r == 1, r != 2, &k);
    expect((l == 1 || r == 1) ? (k && o) : (l == 2 || r == 2) ? !k : (k && !o), "three-valued OR");
  }
  // ---- the evaluator: edge cells × a corpus of programs
  const int64_t ints[] = {0, 1, -1, INT64_MIN, INT64_MAX, (1ll << 53) + 1};
  const double floats[] = {0.0, -0.0, 1.5, nan, inf, -inf, 9007199254740992.0};
  const char *strs[] = {"", "a", "ab", "b"};
  std::vector<Row> rows;
  for (int n = 0; n < 64; ++n) {
    Row r;
    r.c[0].cls = kPvInteger; r.c[0].is_null = n % 7 == 0; r.c[0].i = ints[n % 6];
    r.c[1].cls = kPvFloat; r.c[1].is_null = n % 5 == 0; r.c[1].f = floats[n % 7];
    r.c[2].cls = kPvString; r.c[2].is_null = n % 4 == 0; r.c[2].s = strs[n % 4];
    r.c[3].cls = kPvDate32; r.c[3].is_null = n % 3 == 0; r.c[3].i = 9000 + n % 3;
    r.c[4].cls = kPvInteger; r.c[4].is_null = false; r.c[4].i = n % 5 - 2;
    rows.push_back(r);
  }
  const Program x{column(1)}, y{column(2)}, s{column(3)}, d{column(4)}, c{column(5)};
  std::vector<Program> leaves{x, y, c, {lit_i(0)}, {lit_f(nan)}, {lit_null()}, s, d, {lit_s("a")}, {lit_date(9001)}};
  std::vector<Program> corpus;
  for (const Program &l : leaves) {
    corpus.push_back(cat({l, {tok(LLKV_TOK_NOT)}}));
    corpus.push_back(cat({l, {tok(LLKV_TOK_IS_NULL, 1)}}));
    corpus.push_back(cat({l, {tok(LLKV_TOK_CAST, LLKV_DT_INT64)}}));
    corpus.push_back(cat({l, {tok(LLKV_TOK_CAST, LLKV_DT_FLOAT32)}}));
    corpus.push_back(cat({l, {tok(LLKV_TOK_CAST, LLKV_DT_UTF8)}}));
    for (const Program &r : leaves) {
      for (int op = 0; op <= 7; ++op) corpus.push_back(cat({l, r, {tok(LLKV_TOK_COMPARE, op)}}));
      for (int op = 1; op <= 8; ++op) corpus.push_back(cat({l, r, {tok(LLKV_TOK_BINARY, op)}}));
      corpus.push_back(cat({l, r, {tok(LLKV_TOK_COALESCE, 0, 2)}}));
      corpus.push_back(cat({l, r, {tok(LLKV_TOK_CASE, 0, 1)}}));                                   // searched, no ELSE
      corpus.push_back(cat({l, r, c, {tok(LLKV_TOK_CASE, LLKV_CASE_HAS_ELSE, 1)}}));
      corpus.push_back(cat({l, r, c, {tok(LLKV_TOK_CASE, LLKV_CASE_HAS_OPERAND, 1)}}));           // simple: operand l, candidate r
      corpus.push_back(cat({l, r, y, x, c, {tok(LLKV_TOK_CASE, LLKV_CASE_HAS_OPERAND | LLKV_CASE_HAS_ELSE, 2)}}));
    }
  }
  // malformed and beyond the caps
  corpus.push_back({tok(LLKV_TOK_CASE, 3, 1)});
  corpus.push_back({column(1), tok(LLKV_TOK_CASE, 0, 0)});
  corpus.push_back({column(1), tok(LLKV_TOK_CASE, 0, 9)});
  corpus.push_back({column(1), tok(LLKV_TOK_COALESCE, 0, 0)});
  corpus.push_back({column(1), tok(LLKV_TOK_COALESCE, 0, 4000000000u)});
  corpus.push_back({column(1), column(1)});
  corpus.push_back({column(9)});
  corpus.push_back({tok(42)});
  corpus.push_back({lit_s(nullptr)});
  corpus.push_back(Program(65, lit_i(1)));
  corpus.push_back({});
  size_t values = 0, refusals = 0;
  for (const Program &p : corpus)
    for (const Row &r : rows) {
      CondValue v;
      std::string err;
      const int rc = eval(p, r, &v, &err);
      if (rc) { ++refusals; expect(!err.empty() && (rc == LLKV_INVALID_ARGUMENT || rc == LLKV_UNSUPPORTED || rc == LLKV_NOT_FOUND), "a refusal carries a status and words"); }
      else { ++values; expect(v.cls == kPvNull || v.cls == kPvInteger || v.cls == kPvFloat, "a value is Null, Integer or Float"); }
    }
  // a few pinned rows through the evaluator
  {
    Row r = rows[1]; // x = 1, y = -0.0, s = "a", c = -1
    CondValue v;
    std::string err;
    const Program pivot = cat({x, {lit_i(1)}, {tok(LLKV_TOK_COMPARE, LLKV_CMP_LT_EQ)}, y, {lit_f(0.0)}, {tok(LLKV_TOK_CASE, LLKV_CASE_HAS_ELSE, 1)}});
    expect(eval(pivot, r, &v, &err) == 0 && v.cls == kPvFloat && std::signbit(v.f), "CASE WHEN x <= 1 THEN y ELSE 0.0 END keeps y's bits");
    const Program mixed = cat({x, y, {lit_i(0)}, {tok(LLKV_TOK_CASE, LLKV_CASE_HAS_ELSE, 1)}});
    expect(eval(mixed, r, &v, &err) == LLKV_UNSUPPORTED && err.find("mixed classes") != std::string::npos, "mixed branches are refused");
    const Program str = cat({s, {lit_s("ab")}, {tok(LLKV_TOK_COMPARE, LLKV_CMP_LT)}});
    expect(eval(str, r, &v, &err) == 0 && v.cls == kPvInteger && v.i == 1, "'a' < 'ab' by bytes, then length");
    const Program dates = cat({d, {lit_date(9001)}, {tok(LLKV_TOK_COMPARE, LLKV_CMP_EQ)}});
    expect(eval(dates, r, &v, &err) == 0 && v.cls == kPvInteger && v.i == 0, "Date32 against Date32 is Integer 0");
  }
  std::printf("planvalue_rules_check: %zu programs x %zu rows: %zu values, %zu refusals, %d mismatches\n", corpus.size(), rows.size(), values, refusals, failures);
  return failures ? 1 : 0;
}
