// plan_dump.cpp — differential dump of the host-side plan lowering (csrc/plan.cpp).  Lowers an enumerated corpus through the
// six lower_* entry points, cast_literal_for_column, dictionary_ranks and parse_numeric_or_zero and writes one canonical text
// record per case (entry point, flags, status, error text, every field of the LoweredPlan; doubles as bit patterns).  Two
// builds — one against an older plan.cpp, one against the tree's — must write byte-identical dumps.  Includes plan.hpp only.
//   g++ -std=c++17 -O2 -I include -I rust-llkv_amd/csrc -o tools/plan_dump tools/plan_dump.cpp rust-llkv_amd/csrc/plan.cpp rust-llkv_amd/csrc/planvalue_expr.cpp
//   tools/plan_dump > dump.txt                                  the records; per-entry-point counts on stderr
//   tools/plan_dump --coverage-report plan.cpp jit_seed_plans.txt   which node names / fail() messages of that source the corpus reaches
//   tools/plan_dump --time                                      median host time of seven representative lowerings
#include "plan.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <map>
#include <set>
#include <sstream>

using namespace llkv;
typedef __int128 i128;
using Expr = std::vector<llkv_expr_token>;

// ---------------------------------------------------------------- output
static FILE *g_out = stdout;
static bool g_quiet = false; // coverage / time modes: lower, collect, write nothing
static std::map<std::string, size_t> g_counts;
static std::set<std::string> g_nodes, g_errs;
static std::string g_env = "-";
static bool g_exact = false;
static size_t g_index = 0;

static uint64_t fnv(const void *p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t *)p)[i]) * 1099511628211ull;
  return h;
}
template <class T> static void vec(const char *name, const std::vector<T> &v) {
  if (g_quiet) return;
  fprintf(g_out, " %s[%zu]", name, v.size());
  if (v.size() > 64) { fprintf(g_out, "#%016llx", (unsigned long long)fnv(v.data(), v.size() * sizeof(T))); return; }
  for (const T &x : v) {
    if (sizeof(T) == 8) { uint64_t b; memcpy(&b, &x, 8); fprintf(g_out, ",%llx", (unsigned long long)b); }
    else fprintf(g_out, ",%lld", (long long)x);
  }
}
static void note_nodes(const std::string &ts) {
  for (size_t i = 0; i < ts.size();) {
    if (!isalpha((unsigned char)ts[i])) { ++i; continue; }
    size_t j = i;
    while (j < ts.size() && isalnum((unsigned char)ts[j])) ++j;
    g_nodes.insert(ts.substr(i, j - i));
    i = j;
  }
}
static void dump_plan(const LoweredPlan &p) {
  note_nodes(p.type_string);
  if (g_quiet) { if (p.distinct_proj) dump_plan(*p.distinct_proj); return; }
  fprintf(g_out, " ts=%s\n", p.type_string.c_str());
  vec("sf", p.slot_fields); vec("sd", p.slot_dtypes); vec("sv", p.slot_is_valid); vec("li", p.lit_i); vec("lf", p.lit_f);
  vec("kf", p.key_fields); vec("ks", p.key_slots); vec("kst", p.key_strides); vec("kc", p.key_cards); vec("kb", p.key_bases);
  vec("ki", p.key_is_int); vec("kn", p.key_nullable);
  fprintf(g_out, "\n late=%d ng=%u gr=%d tf=%d lds=%d img=%d part=%d passes=%d c32=%d kimg=%d mingrid=%u df=%lld dn=%u k=%d lanes=%d un=%d bpr=%llu af=%d at=%d dnode=%s",
          p.late_columns, p.ng, p.grouped, p.track_first, p.acc_lds, p.acc_image, p.acc_part, p.image_passes, p.image_cell32, p.k_image, p.image_min_grid,
          (long long)p.distinct_field, p.distinct_numeric, p.k, p.lanes, p.unroll, (unsigned long long)p.bytes_per_row, p.always_false, p.always_true, p.distinct_node.c_str());
  vec("isrc", p.image_src); vec("ixf", p.image_xf); vec("ddn", p.distinct_dict_num); vec("ops", p.lane_ops);
  vec("od", p.out_dtypes); vec("ow", p.out_wide); vec("of", p.out_fields); vec("on", p.out_nullable); vec("cb", p.code_bits);
  for (auto &d : p.dict_num) { fprintf(g_out, " dictnum@%d", d.first); vec("", d.second); }
  fprintf(g_out, " dtok[%zu]", p.distinct_tokens.size());
  for (auto &t : p.distinct_tokens) {
    uint64_t fb; memcpy(&fb, &t.literal.f64, 8);
    fprintf(g_out, ",%d/%d/%u/%d/%d/%llx/%llx/%llx/%d", t.kind, t.binop, t.field_id, t.literal.tag, t.literal.scale, (unsigned long long)t.literal.lo, (unsigned long long)t.literal.hi,
            (unsigned long long)fb, t.literal.str != nullptr);
  }
  fprintf(g_out, "\n");
  for (const AggOut &a : p.aggs) {
    fprintf(g_out, " agg fin=%d lane=%d tbf=%d fast=%d wide=%d plain=%d nwv=%d wd=%d wb=%llx/%llx prec=%d sc=%d dl=%d ds=%d cl=%d xl=%d fp=%d fe=%d nd=%d\n", (int)a.fin, a.lane,
            a.typed_by_first_value, a.fast_sum, a.wide, a.plain_minmax, a.null_without_values, a.wide_delta, (unsigned long long)a.wide_base_hi, (unsigned long long)a.wide_base_lo,
            a.precision, a.scale, a.digits_lane, a.digits_shift, a.count_lane, a.exact_levels, a.fixed_point, a.fixed_exp, a.nan_default);
  }
  if (p.distinct_proj) { fprintf(g_out, " distinct_proj:"); dump_plan(*p.distinct_proj); }
}
static void record(const char *entry, const std::string &name, int rc, const std::string &err, const LoweredPlan *p, const std::string &extra = "") {
  ++g_counts[entry];
  ++g_index;
  if (rc) g_errs.insert(err);
  if (!g_quiet) fprintf(g_out, "#%zu %s %s env=%s exact=%d rc=%d err=%s %s\n", g_index, entry, name.c_str(), g_env.c_str(), g_exact, rc, rc ? err.c_str() : "", extra.c_str());
  if (!rc && p) dump_plan(*p);
}

// ---------------------------------------------------------------- catalogue
static std::vector<ColumnInfo> g_cols;
static const ColumnInfo *resolve_fn(uint32_t f) { return f >= 1 && f <= g_cols.size() ? &g_cols[f - 1] : nullptr; }
static const ColumnResolver g_resolve = resolve_fn;
static uint32_t add_col(ColumnInfo c) { c.field_id = (uint32_t)g_cols.size() + 1; g_cols.push_back(c); return c.field_id; }
static const uint64_t kRows[] = {1000, 6000000, (1ull << 31) - 1, 1ull << 31, (1ull << 32) - 1, (1ull << 32) + 1, (1ull << 38) - 1, (1ull << 38) + 1, 0};
static const uint32_t kMissing = 99999;

static std::vector<std::string> dict_seq(size_t n, const char *fmt) {
  std::vector<std::string> d;
  char b[32];
  for (size_t i = 0; i < n; ++i) { snprintf(b, sizeof b, fmt, (int)i); d.push_back(b); }
  return d;
}
// representative columns (field ids), filled by build_catalogue
static uint32_t cI64, cI64n, cI64ns, cI64big, cI32, cI32n, cU32, cU64, cDate, cF64, cF64n, cF64ns, cF64plain, cF32, cDec2, cDec0n, cDec4, cDecWide, cDecWideBig, cDecBadScale,
    cUtfNum, cUtfKey, cUtfKeyN, cUtf256, cUtfWide, cUtfWideN, cUtfBig, cUtfNonAscii, cBool, cBoolN, cNullT, cI64key, cI64keyN, cI32key, cDateKey, cI64range, cU64b;

static void build_catalogue() {
  size_t r = 0;
  auto rows = [&]() { return kRows[r++ % 9]; };
  const int32_t ints[] = {LLKV_DT_INT64, LLKV_DT_INT32, LLKV_DT_DATE32, LLKV_DT_UINT64, LLKV_DT_UINT32, LLKV_DT_BOOLEAN, LLKV_DT_NULL, 42};
  for (int32_t dt : ints)
    for (int nullable = 0; nullable < 2; ++nullable)
      for (int st = 0; st < 4; ++st) {
        ColumnInfo c;
        c.dtype = dt; c.nullable = nullable; c.rows = rows(); c.ascending = st == 1;
        c.has_stats = st != 0;
        if (st == 1) { c.min_i = -5; c.max_i = 100; }
        if (st == 2) { c.min_i = -(1ll << 60); c.max_i = (1ll << 55) + 3; }
        if (st == 3) { c.min_i = INT64_MIN; c.max_i = INT64_MAX; }
        add_col(c);
      }
  for (int32_t dt : {LLKV_DT_FLOAT64, LLKV_DT_FLOAT32})
    for (int nullable = 0; nullable < 2; ++nullable) {
      ColumnInfo c;
      c.dtype = dt; c.nullable = nullable; c.rows = rows();
      add_col(c);
      for (int flags = 0; flags < 8; ++flags)
        for (double mn : {0.0, 4.9406564584124654e-324, 0.01, 3.0}) {
          c.has_fstats = true; c.f_all_finite = flags & 1; c.f_no_neg_zero = flags & 2; c.f_no_nan = flags & 4;
          c.f_absmax = mn == 3.0 ? 1e300 : 104949.5; c.f_absmin_nz = mn; c.rows = rows();
          add_col(c);
        }
      c.f_absmax = 0.0; c.f_absmin_nz = 0.0; add_col(c); // an all-zero column
      c.f_absmax = INFINITY; add_col(c);
    }
  for (int scale : {-39, -38, -2, 0, 2, 18, 19, 38, 39})
    for (int nullable = 0; nullable < 2; ++nullable)
      for (int st = 0; st < 3; ++st) {
        ColumnInfo c;
        c.dtype = LLKV_DT_DECIMAL128; c.precision = 15; c.scale = scale; c.nullable = nullable; c.rows = rows();
        c.has_stats = st != 0;
        if (st == 1) { c.min_i = 0; c.max_i = 10494950; }
        if (st == 2) { c.min_i = INT64_MIN + 1; c.max_i = INT64_MAX; }
        add_col(c);
      }
  for (int span = 0; span < 4; ++span)
    for (int nullable = 0; nullable < 2; ++nullable)
      for (uint64_t rws : {(uint64_t)1000, (uint64_t)1 << 31, (uint64_t)1 << 20}) {
        ColumnInfo c;
        c.dtype = LLKV_DT_DECIMAL128; c.precision = 38; c.scale = 4; c.nullable = nullable; c.rows = rws; c.wide128 = true;
        c.wide_min_hi = 5; c.wide_min_lo = 100; c.wide_max_hi = span == 0 ? 5 : span == 1 ? 6 : span == 2 ? 9 : 4; c.wide_max_lo = span == 1 ? 99 : 7000;
        c.wide_absmax_hi = span == 2 ? (1ull << 62) : 9; c.wide_absmax_lo = 1;
        add_col(c);
      }
  const std::vector<std::vector<std::string>> dicts = {{}, {"1", " 2.5 ", "abc", "-3e2", "+.5", "1e", "0x10"}, {"7", "inf", "NaN"}, {"A", "F", "N", "O", "R"}, {"\xC3\xA9t\xC3\xA9", "Z\xC3\xBCrich", "abc", "ABC"},
                                                       dict_seq(256, "s%03d"), dict_seq(257, "s%03d"), dict_seq(3000, "k%04d"), dict_seq(300, "%d")};
  for (auto &d : dicts)
    for (int nullable = 0; nullable < 2; ++nullable) {
      ColumnInfo c;
      c.dtype = LLKV_DT_UTF8; c.nullable = nullable; c.rows = rows(); c.dictionary = d;
      if (d.size() > 256) std::sort(c.dictionary.begin(), c.dictionary.end());
      add_col(c);
    }
  { ColumnInfo c; c.dtype = LLKV_DT_UTF8; c.rows = 500; c.dictionary = dict_seq(3000, "k%04d"); c.dictionary[7] = "k\xC3\xA9"; std::sort(c.dictionary.begin(), c.dictionary.end()); cUtfNonAscii = add_col(c); }
  // the representatives, with fixed row counts
  auto mk = [&](int32_t dt, bool nullable, int st, uint64_t rws) {
    ColumnInfo c;
    c.dtype = dt; c.nullable = nullable; c.rows = rws; c.has_stats = st != 0;
    if (st == 1) { c.min_i = 1; c.max_i = 50; }
    if (st == 2) { c.min_i = -(1ll << 60); c.max_i = 1ll << 60; }
    if (st == 3) { c.min_i = 0; c.max_i = 99999; }
    return c;
  };
  cI64 = add_col(mk(LLKV_DT_INT64, false, 1, 6000000)); cI64n = add_col(mk(LLKV_DT_INT64, true, 1, 6000000)); cI64ns = add_col(mk(LLKV_DT_INT64, false, 0, 6000000));
  cI64big = add_col(mk(LLKV_DT_INT64, false, 2, 6000000)); cI32 = add_col(mk(LLKV_DT_INT32, false, 1, 6000000)); cI32n = add_col(mk(LLKV_DT_INT32, true, 0, 1000));
  cU32 = add_col(mk(LLKV_DT_UINT32, false, 1, 6000000)); cU64 = add_col(mk(LLKV_DT_UINT64, false, 1, 6000000)); cU64b = add_col(mk(LLKV_DT_UINT64, false, 0, 6000000));
  cDate = add_col(mk(LLKV_DT_DATE32, false, 3, 6000000));
  { ColumnInfo c = mk(LLKV_DT_FLOAT64, false, 0, 6000000); c.has_fstats = true; c.f_all_finite = c.f_no_nan = true; c.f_absmax = 104949.5; c.f_absmin_nz = 0.01; cF64 = add_col(c);
    c.nullable = true; cF64n = add_col(c); c.nullable = false; c.f_no_neg_zero = true; c.rows = 1000; cF64plain = add_col(c); }
  cF64ns = add_col(mk(LLKV_DT_FLOAT64, false, 0, 6000000));
  { ColumnInfo c = mk(LLKV_DT_FLOAT32, false, 0, 6000000); c.has_fstats = true; c.f_all_finite = true; c.f_absmax = 10.0; c.f_absmin_nz = 0.5; cF32 = add_col(c); }
  auto dec = [&](int scale, bool nullable, int st) { ColumnInfo c = mk(LLKV_DT_DECIMAL128, nullable, st, 6000000); c.precision = 15; c.scale = scale; return c; };
  cDec2 = add_col(dec(2, false, 3)); cDec0n = add_col(dec(0, true, 1)); cDec4 = add_col(dec(4, false, 2)); cDecBadScale = add_col(dec(40, false, 1));
  cDecWide = (uint32_t)0; cDecWideBig = 0;
  for (auto &c : g_cols) if (c.wide128 && !c.nullable && c.rows == 1000) { if (c.wide_max_hi == 5) cDecWide = c.field_id; if (c.wide_max_hi == 9) cDecWideBig = c.field_id; }
  auto utf = [&](std::vector<std::string> d, bool nullable, uint64_t rws) { ColumnInfo c = mk(LLKV_DT_UTF8, nullable, 0, rws); c.dictionary = d; return c; };
  cUtfNum = add_col(utf({"1", " 2.5 ", "abc", "-3e2"}, false, 6000000)); cUtfKey = add_col(utf({"A", "N", "R"}, false, 6000000)); cUtfKeyN = add_col(utf({"F", "O"}, true, 6000000));
  cUtf256 = add_col(utf(dict_seq(256, "s%03d"), false, 6000000)); cUtfWide = add_col(utf(dict_seq(3000, "k%04d"), false, 6000000)); cUtfWideN = add_col(utf(dict_seq(300, "w%03d"), true, 6000000));
  cUtfBig = add_col(utf(dict_seq(70000, "b%05d"), false, 6000000));
  cBool = add_col(mk(LLKV_DT_BOOLEAN, false, 0, 6000000)); cBoolN = add_col(mk(LLKV_DT_BOOLEAN, true, 0, 6000000)); cNullT = add_col(mk(LLKV_DT_NULL, false, 0, 1000));
  cI64key = add_col(mk(LLKV_DT_INT64, false, 1, 6000000)); cI64keyN = add_col(mk(LLKV_DT_INT64, true, 1, (1ull << 32) + 5)); cI32key = add_col(mk(LLKV_DT_INT32, false, 1, 6000000));
  cDateKey = add_col(mk(LLKV_DT_DATE32, true, 1, 6000000)); cI64range = add_col(mk(LLKV_DT_INT64, false, 3, 6000000));
}

// ---------------------------------------------------------------- expressions
struct E { Expr t; std::string name; };
static llkv_literal lit_int(i128 v) { llkv_literal l{}; l.tag = LLKV_LIT_INT128; l.lo = (uint64_t)v; l.hi = (int64_t)(v >> 64); return l; }
static llkv_literal lit_f64(double v) { llkv_literal l{}; l.tag = LLKV_LIT_FLOAT64; l.f64 = v; return l; }
static llkv_literal lit_dec(i128 v, int scale) { llkv_literal l = lit_int(v); l.tag = LLKV_LIT_DECIMAL128; l.scale = scale; return l; }
static llkv_literal lit_tag(int tag, uint64_t lo = 0) { llkv_literal l{}; l.tag = tag; l.lo = lo; return l; }
static llkv_literal lit_str(const char *s) { llkv_literal l{}; l.tag = LLKV_LIT_STRING; l.str = s; return l; }
static E col(uint32_t f) { llkv_expr_token t{}; t.kind = LLKV_TOK_COLUMN; t.field_id = f; return {{t}, "c" + std::to_string(f)}; }
static E lit(const llkv_literal &l, const std::string &name) { llkv_expr_token t{}; t.kind = LLKV_TOK_LITERAL; t.literal = l; return {{t}, name}; }
static E bin(int op, const E &l, const E &r) {
  E o = l;
  o.t.insert(o.t.end(), r.t.begin(), r.t.end());
  llkv_expr_token t{}; t.kind = LLKV_TOK_BINARY; t.binop = op;
  o.t.push_back(t);
  static const char *names[] = {"?0", "+", "-", "*", "/", "%", "?6"};
  o.name = "(" + l.name + names[op < 0 || op > 6 ? 0 : op] + r.name + ")";
  return o;
}
static std::vector<E> operands_full, operands_mid, operands_small, operands_tiny, exprs1, exprs23;
static void build_expressions() {
  const i128 huge = ((i128)1 << 100);
  std::vector<E> lits = {lit(lit_int(3), "3"), lit(lit_int(0), "0"), lit(lit_int(-1), "-1"), lit(lit_int(INT64_MIN), "imin"), lit(lit_int(huge), "huge"), lit(lit_int((i128)1 << 62), "2^62"),
                         lit(lit_f64(1.5), "1.5"), lit(lit_f64(0.0), "0.0"), lit(lit_f64(-0.0), "-0.0"), lit(lit_f64(NAN), "nan"), lit(lit_f64(INFINITY), "inf"),
                         lit(lit_dec(150, 2), "d1.50"), lit(lit_dec(huge, 2), "dhuge"), lit(lit_dec(7, -3), "d7e3"), lit(lit_dec(1, 39), "ds39"), lit(lit_tag(LLKV_LIT_NULL), "null"),
                         lit(lit_str("x"), "'x'"), lit(lit_tag(LLKV_LIT_BOOLEAN, 1), "true"), lit(lit_tag(LLKV_LIT_DATE32, 9000), "date")};
  for (uint32_t f : {cI64, cI64n, cI64ns, cI64big, cI32, cI32n, cU32, cU64, cU64b, cDate, cF64, cF64n, cF64ns, cF32, cDec2, cDec0n, cDec4, cDecBadScale, cDecWide, cUtfNum, cUtfWide, cBool, cNullT, kMissing})
    operands_full.push_back(col(f));
  operands_full.insert(operands_full.end(), lits.begin(), lits.end());
  for (uint32_t f : {cI64, cI64n, cI64ns, cI64big, cI32, cU32, cU64, cF64, cF64n, cF32, cDec2, cDec0n, cDec4, cUtfNum}) operands_mid.push_back(col(f));
  for (int i : {0, 1, 2, 3, 6, 7, 11, 13, 15}) operands_mid.push_back(lits[i]);
  for (uint32_t f : {cI64, cI64n, cF64, cDec2}) operands_small.push_back(col(f));
  for (int i : {0, 1, 6}) operands_small.push_back(lits[i]);
  operands_tiny = {col(cI64n), col(cF64), col(cDec2), lits[0], lits[1]};
  for (auto &a : operands_mid) for (auto &b : operands_mid) for (int op = 1; op <= 5; ++op) exprs1.push_back(bin(op, a, b));
  exprs1.push_back(bin(6, col(cI64), lits[0])); exprs1.push_back(bin(0, lits[0], lits[0])); // an operator outside the vocabulary
  { E under = col(cI64); llkv_expr_token t{}; t.kind = LLKV_TOK_BINARY; t.binop = 1; under.t.push_back(t); under.name = "underflow"; exprs1.push_back(under); }
  { E two = col(cI64); two.t.push_back(two.t[0]); two.name = "two-results"; exprs1.push_back(two); }
  { E d = bin(4, col(cF64), col(cI64)); d.t.push_back(d.t[0]); d.name = "div-two-results"; exprs1.push_back(d); E u = col(cI64); llkv_expr_token t{}; t.kind = LLKV_TOK_BINARY; t.binop = 4; u.t.push_back(t); u.name = "div-underflow"; exprs1.push_back(u); }
  { // decimal scales at the edges: a product scale beyond 38, a rescale by more than 18 digits; a string literal behind a division
    uint32_t s38 = 0, sm2 = 0, s18 = 0;
    for (auto &c : g_cols) if (c.dtype == LLKV_DT_DECIMAL128 && !c.wide128 && c.has_stats && c.min_i == 0 && !c.nullable) { if (c.scale == 38) s38 = c.field_id; if (c.scale == -2) sm2 = c.field_id; if (c.scale == 18) s18 = c.field_id; }
    for (int op = 1; op <= 5; ++op) { exprs1.push_back(bin(op, col(s38), col(cDec2))); exprs1.push_back(bin(op, col(sm2), col(s18))); exprs1.push_back(bin(op, col(sm2), col(cDec2))); }
    exprs1.push_back(bin(1, bin(4, col(cI64), col(cI64)), lits[16]));
  }
  for (uint32_t f : {cI32, cU32}) for (uint32_t g : {cI32, cU32, cI32n}) for (int op = 1; op <= 5; ++op) exprs1.push_back(bin(op, col(f), col(g)));
  for (auto &a : operands_small) for (auto &b : operands_small) for (auto &c : operands_small) for (int o1 = 1; o1 <= 5; ++o1) for (int o2 = 1; o2 <= 5; ++o2) {
    exprs23.push_back(bin(o2, bin(o1, a, b), c));
    exprs23.push_back(bin(o2, a, bin(o1, b, c)));
  }
  for (auto &a : operands_tiny) for (auto &b : operands_tiny) for (auto &c : operands_tiny) for (auto &d : operands_tiny)
    for (int o1 : {1, 4}) for (int o2 : {3, 4, 5}) for (int o3 : {2, 3}) {
      exprs23.push_back(bin(o3, bin(o2, bin(o1, a, b), c), d));
      exprs23.push_back(bin(o2, bin(o1, a, b), bin(o3, c, d)));
    }
}

// ---------------------------------------------------------------- entry-point wrappers
static llkv_filter leaf(uint32_t field, int op, const llkv_literal &v = llkv_literal{}) { llkv_filter f{}; f.field_id = field; f.op = op; f.value = v; f.case_sensitive = 1; return f; }
static llkv_filter compare(int op, const E &l, const E &r) { llkv_filter f{}; f.op = LLKV_OP_COMPARE; f.cmp_op = op; f.cmp_left = l.t.data(); f.cmp_left_len = (uint32_t)l.t.size(); f.cmp_right = r.t.data(); f.cmp_right_len = (uint32_t)r.t.size(); return f; }
static llkv_aggregate_spec agg(int kind, int distinct, const E *e) { llkv_aggregate_spec s{}; s.kind = kind; s.distinct = distinct; if (e) { s.expr = e->t.data(); s.expr_len = (uint32_t)e->t.size(); } return s; }

static void sel(const std::string &name, const std::vector<llkv_filter> &fs, const std::vector<llkv_eval_op> &ops = {}, const std::vector<uint32_t> &drop = {}) {
  LoweredPlan p; std::string err;
  int rc = lower_selection(g_resolve, fs.data(), (uint32_t)fs.size(), ops.data(), (uint32_t)ops.size(), drop.data(), (uint32_t)drop.size(), &p, &err);
  record("selection", name, rc, err, &p);
}
static void plan(const std::string &name, const std::vector<llkv_filter> &fs, const std::vector<uint32_t> &keys, const std::vector<llkv_aggregate_spec> &aggs, int flags,
                 const std::vector<llkv_eval_op> &ops = {}) { // flags: 1 grouped, 2 track_first, 4 image, 8 partitioned
  LoweredPlan p; std::string err;
  int rc = lower_plan(g_resolve, fs.data(), (uint32_t)fs.size(), ops.data(), (uint32_t)ops.size(), keys.data(), (uint32_t)keys.size(), aggs.data(), (uint32_t)aggs.size(), flags & 1, flags & 2, &p, &err,
                      flags & 4, flags & 8);
  record("plan", name + " f" + std::to_string(flags), rc, err, &p);
}
static void reduce(const std::string &name, const std::vector<llkv_aggregate_spec> &aggs) {
  LoweredPlan p; std::string err;
  int rc = lower_reduce(g_resolve, aggs.data(), (uint32_t)aggs.size(), &p, &err);
  record("reduce", name, rc, err, &p);
}
static void proj(const std::string &name, const std::vector<llkv_projection> &ps, bool pad) {
  LoweredPlan p; std::string err;
  int rc = lower_projection(g_resolve, ps.data(), (uint32_t)ps.size(), &p, &err, pad);
  record("projection", name + (pad ? " pad" : ""), rc, err, &p);
}
static void emit(const std::string &name, const std::vector<llkv_filter> &fs, const E &e, int flags, const uint32_t *in_set = nullptr, const std::vector<llkv_eval_op> &ops = {}) {
  LoweredPlan p; std::string err; // flags: 1 allow_f64, 2 key_dtype wanted, 4 int32_value, 8 is_f64 wanted
  bool is_f64 = false; int32_t kd = -7;
  int rc = lower_emit(g_resolve, fs.data(), (uint32_t)fs.size(), ops.data(), (uint32_t)ops.size(), e.t.data(), (uint32_t)e.t.size(), &p, &err, flags & 1, flags & 8 ? &is_f64 : nullptr, in_set,
                      flags & 2 ? &kd : nullptr, flags & 4);
  record("emit", name + " " + e.name + " f" + std::to_string(flags) + (in_set ? " set" + std::to_string(*in_set) : ""), rc, err, &p, "isf=" + std::to_string(is_f64) + " kd=" + std::to_string(kd));
}
static void probe(const std::string &name, const std::vector<llkv_filter> &fs, uint32_t key, const E *e, bool keybit) {
  LoweredPlan p; std::string err;
  int rc = lower_probe(g_resolve, fs.data(), (uint32_t)fs.size(), key, e ? e->t.data() : nullptr, e ? (uint32_t)e->t.size() : 0, &p, &err, keybit);
  record("probe", name + " k" + std::to_string(key) + " " + (e ? e->name : "noexpr") + (keybit ? " keybit" : ""), rc, err, &p);
}
static void in_set(const std::string &name, const std::vector<llkv_filter> &fs, uint32_t key) {
  LoweredPlan p; std::string err;
  int rc = lower_selection_in_set(g_resolve, fs.data(), (uint32_t)fs.size(), key, &p, &err);
  record("selection_in_set", name + " k" + std::to_string(key), rc, err, &p);
}

// ---------------------------------------------------------------- the corpus
static std::deque<std::string> g_keep; // string literals the filters borrow
static std::vector<llkv_literal> leaf_literals() {
  return {lit_int(5), lit_int(-1), lit_int((i128)1 << 40), lit_int((i128)1 << 70), lit_f64(1.5), lit_f64(1e40), lit_f64(NAN), lit_dec(500, 2), lit_dec(5, 0), lit_dec(0, 3), lit_tag(LLKV_LIT_NULL),
          lit_tag(LLKV_LIT_BOOLEAN, 1), lit_tag(LLKV_LIT_DATE32, 9000), lit_str("s010"), lit_str("k1500"), lit_str("abc"), lit_str("N"), lit_str("\xC3\x89"), lit_str(""), lit_str(nullptr)};
}
static std::vector<uint32_t> all_fields() { std::vector<uint32_t> v; for (auto &c : g_cols) v.push_back(c.field_id); v.push_back(kMissing); return v; }
static std::vector<uint32_t> rep_fields() {
  return {cI64, cI64n, cI64ns, cI64big, cI32, cI32n, cU32, cU64, cDate, cF64, cF64n, cF64ns, cF64plain, cF32, cDec2, cDec0n, cDec4, cDecWide, cDecWideBig, cUtfNum, cUtfKey, cUtfKeyN, cUtf256,
          cUtfWide, cUtfWideN, cBool, cBoolN, cNullT, cI64key, cI64keyN, kMissing};
}

static void leaves_of(uint32_t f, bool through_emit) {
  const std::string n = "leaf c" + std::to_string(f);
  auto run = [&](const std::string &nm, const llkv_filter &fl) {
    sel(nm, {fl});
    if (through_emit) { emit(nm, {fl}, col(cI64), 0); plan(nm, {fl}, {cUtfKey}, {agg(LLKV_AGG_COUNT_STAR, 0, nullptr)}, 1 | 4); }
  };
  const auto lits = leaf_literals();
  for (int op : {1, 3, 4, 5, 6, 8, 9, 14, 15, 16, 0, 77})
    for (size_t i = 0; i < lits.size(); ++i) {
      if ((op == 8 || op == 9) && i) break;
      for (int cs = 1; cs >= (op >= 14 && op <= 16 ? 0 : 1); --cs) {
        llkv_filter fl = leaf(f, op, lits[i]);
        fl.case_sensitive = cs;
        run(n + " op" + std::to_string(op) + " l" + std::to_string(i) + (cs ? "" : " ci"), fl);
      }
    }
  for (const char *pat : {"S0", "K1", "k00", "9", "\xC3\xA9"})
    for (int op = 14; op <= 16; ++op)
      for (int cs = 0; cs < 2; ++cs) { llkv_filter fl = leaf(f, op, lit_str(pat)); fl.case_sensitive = cs; run(n + " pat" + pat + " op" + std::to_string(op) + " cs" + std::to_string(cs), fl); }
  const llkv_literal bounds[][2] = {{lit_int(1), lit_int(50)}, {lit_str("s010"), lit_str("s100")}, {lit_f64(0.5), lit_f64(2.5)}, {lit_str("k0000"), lit_str("k9999")}, {lit_str("k2000"), lit_str("k1000")},
                                    {lit_int(1), lit_str("x")}, {lit_str("x"), lit_int(1)}, {lit_int((i128)1 << 70), lit_int(1)}, {lit_int(1), lit_int((i128)1 << 70)}};
  for (auto &b : bounds)
    for (int lk = 0; lk < 3; ++lk)
      for (int uk = 0; uk < 3; ++uk) {
        llkv_filter fl = leaf(f, LLKV_OP_RANGE);
        fl.lower_kind = lk; fl.lower = b[0]; fl.upper_kind = uk; fl.upper = b[1];
        run(n + " range" + std::to_string(&b - bounds) + " " + std::to_string(lk) + std::to_string(uk), fl);
      }
  std::vector<std::vector<llkv_literal>> lists = {{}, {lit_int(5)}, {lit_int(5), lit_int(6), lit_int(5)}, {lit_int(5), lit_tag(LLKV_LIT_NULL)}, {lit_f64(1.5), lit_int(2)}, {lit_str("zz")}, {lit_str("abc"), lit_str("N"), lit_str("1")}};
  for (size_t n_codes : {7, 8, 9, 10, 60}) {
    std::vector<llkv_literal> l;
    for (size_t i = 0; i < n_codes; ++i) {
      char b[16]; snprintf(b, sizeof b, n_codes == 10 ? "s%03d" : "k%04d", (int)(i * 37 % 250));
      g_keep.push_back(b); l.push_back(lit_str(g_keep.back().c_str()));
    }
    lists.push_back(l);
  }
  { std::vector<llkv_literal> l; for (int i = 0; i < 50; ++i) l.push_back(lit_int(i)); lists.push_back(l); l.clear(); for (int i = 0; i < 50; ++i) l.push_back(lit_f64(i + 0.5)); lists.push_back(l); }
  for (size_t i = 0; i < lists.size(); ++i) { llkv_filter fl = leaf(f, LLKV_OP_IN); fl.in_list = lists[i].data(); fl.in_len = (uint32_t)lists[i].size(); run(n + " in" + std::to_string(i), fl); }
}

static void section_leaves() {
  std::set<std::string> shapes; // the leaves read dtype, NULL cells, the dictionary and the decimal form of a column, nothing else
  for (uint32_t f : all_fields()) {
    const ColumnInfo *ci = resolve_fn(f);
    if (ci && !shapes.insert(std::to_string(ci->dtype) + "/" + std::to_string(ci->nullable) + "/" + std::to_string(ci->dictionary.size()) + "/" + std::to_string(ci->wide128) + "/" + std::to_string(ci->scale) + "/" +
                             (ci->dictionary.empty() ? "" : ci->dictionary.back())).second) continue;
    leaves_of(f, ci && (utf8_wide(*ci) || f == cUtfKey || f == cI64 || f == cF64n));
  }
  // MVCC leaf
  std::vector<llkv_literal> ids;
  for (int i = 0; i < 50; ++i) ids.push_back(lit_int(1000 + i));
  for (uint32_t created : {cU64, cU64b, cI64, kMissing})
    for (uint32_t deleted : {cU64b, cU64, cF64, kMissing, cDecWide})
      for (uint32_t n : {0u, 1u, 32u, 33u, 45u, 47u}) {
        llkv_filter fl = leaf(created, LLKV_OP_MVCC_VISIBLE, lit_int(deleted));
        fl.lower = lit_int(7); fl.upper = lit_int(9); fl.in_list = ids.data(); fl.in_len = n;
        sel("mvcc " + std::to_string(created) + "/" + std::to_string(deleted) + " n" + std::to_string(n), {fl});
        if (n == 32) { llkv_filter g = leaf(cI64, LLKV_OP_IN); g.in_list = ids.data(); g.in_len = 20; sel("mvcc+in", {fl, g}); }
      }
}

static void section_compare() {
  const std::vector<E> &O = operands_full;
  for (auto &a : O) for (auto &b : O) for (int op = 0; op <= 7; ++op) {
    if ((op == 0 || op == 7) && (&a != &O[0])) continue;
    sel("cmp" + std::to_string(op) + " " + a.name + " " + b.name, {compare(op, a, b)});
  }
  for (size_t i = 0; i < exprs1.size(); ++i)
    for (const E *b : std::vector<const E *>{&O[0], &O[10], &O[24], &O[30], &O[39], &exprs1[(i * 7 + 3) % exprs1.size()]})
      for (int op : {1, 2, 4}) {
        sel("cmp" + std::to_string(op) + " " + exprs1[i].name + " " + b->name, {compare(op, exprs1[i], *b)});
        if (op == 4) sel("cmp" + std::to_string(op) + " " + b->name + " " + exprs1[i].name, {compare(op, *b, exprs1[i])});
      }
  for (size_t i = 0; i < exprs23.size(); i += 3) sel("cmp3 " + exprs23[i].name, {compare(3, exprs23[i], O[i % O.size()])});
  { llkv_filter f = compare(1, O[0], O[0]); f.cmp_right = nullptr; sel("cmp no right", {f}); f = compare(1, O[0], O[0]); f.cmp_left_len = 0; sel("cmp empty left", {f}); }
  // IN lists
  std::vector<const E *> items = {&O[24], &O[25], &O[30], &O[31], &O[39], &O[0], &O[10], &O[7], &O[40], &O[28], &exprs1[3], &exprs1[40], &exprs1[0], &exprs1[303], &exprs1[78], &O[4], &O[6]};
  std::vector<std::vector<const E *>> lists = {{}};
  for (auto *a : items) lists.push_back({a});
  for (size_t i = 0; i < items.size(); ++i) for (size_t j = i % 3; j < items.size(); j += 3) lists.push_back({items[i], items[j]});
  for (size_t i = 0; i + 2 < items.size(); ++i) lists.push_back({items[i], items[i + 1], items[i + 2]});
  std::vector<const E *> targets;
  for (auto &a : O) targets.push_back(&a);
  for (size_t i = 0; i < exprs1.size(); i += 37) targets.push_back(&exprs1[i]);
  for (auto *t : targets)
    for (size_t li = 0; li < lists.size(); ++li)
      for (int neg = 0; neg < 2; ++neg) {
        std::vector<const llkv_expr_token *> ptrs; std::vector<uint32_t> lens; std::string nm;
        for (auto *e : lists[li]) { ptrs.push_back(e->t.data()); lens.push_back((uint32_t)e->t.size()); nm += " " + e->name; }
        llkv_filter f{}; f.op = LLKV_OP_IN_LIST; f.cmp_left = t->t.data(); f.cmp_left_len = (uint32_t)t->t.size(); f.list_exprs = ptrs.data(); f.list_expr_lens = lens.data(); f.list_len = (uint32_t)ptrs.size(); f.negated = neg;
        sel("inlist " + t->name + (neg ? " not in" : " in") + nm, {f});
      }
  { llkv_filter f{}; f.op = LLKV_OP_IN_LIST; sel("inlist no target", {f}); f.cmp_left = O[0].t.data(); f.cmp_left_len = 1; f.list_len = 2; sel("inlist null arrays", {f}); }
  // IS NULL over expressions
  auto is_null = [&](const E &e, int neg) { llkv_filter f{}; f.op = LLKV_OP_IS_NULL_EXPR; f.cmp_left = e.t.data(); f.cmp_left_len = (uint32_t)e.t.size(); f.negated = neg; sel(std::string("isnull") + (neg ? " not " : " ") + e.name, {f}); };
  for (int neg = 0; neg < 2; ++neg) {
    for (uint32_t f : all_fields()) is_null(col(f), neg);
    for (auto &e : O) is_null(e, neg);
    for (auto &e : exprs1) is_null(e, neg);
    for (size_t i = neg; i < exprs23.size(); i += 5) is_null(exprs23[i], neg);
  }
  { llkv_filter f{}; f.op = LLKV_OP_IS_NULL_EXPR; sel("isnull no expr", {f}); }
}

static void section_programs() {
  static const E e_div = bin(4, col(cI64n), col(cI64)), e_null = lit(lit_tag(LLKV_LIT_NULL), "null"), e_one = lit(lit_int(1), "1"), e_sum = bin(1, col(cF64n), col(cI64n));
  std::vector<llkv_filter> fs = {leaf(cI64, LLKV_OP_GT, lit_int(5)), leaf(cI64n, LLKV_OP_LE, lit_int(7)), leaf(cF64n, LLKV_OP_IS_NULL), leaf(cUtfKeyN, LLKV_OP_EQUALS, lit_str("F")),
                                 compare(3, e_div, e_one), compare(1, e_sum, e_null), compare(1, e_one, e_null), compare(1, e_one, e_one), leaf(cUtfKey, LLKV_OP_EQUALS, lit_str("zz")),
                                 leaf(cI64n, LLKV_OP_RANGE), leaf(cUtfWideN, LLKV_OP_CONTAINS, lit_str("1"))};
  const uint32_t n = (uint32_t)fs.size();
  auto P = [](uint32_t i) { return llkv_eval_op{LLKV_EVAL_PUSH_PREDICATE, i}; };
  const llkv_eval_op NOT{LLKV_EVAL_NOT, 0};
  sel("all_of", fs); sel("none", {});
  for (uint32_t i = 0; i <= n; ++i) {
    sel("push " + std::to_string(i), fs, {P(i)}); sel("not " + std::to_string(i), fs, {P(i), NOT}); sel("notnot " + std::to_string(i), fs, {P(i), NOT, NOT});
    for (uint32_t j = 0; j < n; ++j)
      for (int op : {LLKV_EVAL_AND, LLKV_EVAL_OR})
        for (int v = 0; v < 5; ++v) {
          std::vector<llkv_eval_op> ops = {P(i)};
          if (v == 1) ops.push_back(NOT);
          ops.push_back(P(j));
          if (v == 2) ops.push_back(NOT);
          ops.push_back({op, 2});
          if (v == 3) ops.push_back(NOT);
          if (v == 4) { ops.push_back(P((i + j) % n)); ops.push_back({op == LLKV_EVAL_AND ? LLKV_EVAL_OR : LLKV_EVAL_AND, 2}); }
          const std::string nm = "prog " + std::to_string(i) + (op == LLKV_EVAL_AND ? "&" : "|") + std::to_string(j) + " v" + std::to_string(v);
          sel(nm, fs, ops);
          if (i < n && (i + j) % 3 == 0) { plan(nm, fs, {cUtfKey}, {agg(LLKV_AGG_COUNT_STAR, 0, nullptr)}, 3, ops); emit(nm, fs, col(cI64), 0, nullptr, ops); }
        }
  }
  for (uint32_t lit01 = 0; lit01 < 2; ++lit01) {
    const llkv_eval_op L{LLKV_EVAL_PUSH_LITERAL, lit01};
    sel("lit", fs, {L}); sel("lit not", fs, {L, NOT});
    for (int op : {LLKV_EVAL_AND, LLKV_EVAL_OR}) for (uint32_t i = 0; i < n; ++i) { sel("lit op " + std::to_string(i), fs, {L, P(i), {op, 2}}); sel("lit op3", fs, {L, P(i), P(1), {op, 3}, NOT}); }
  }
  sel("underflow and0", fs, {P(0), {LLKV_EVAL_AND, 0}}); sel("underflow and3", fs, {P(0), P(1), {LLKV_EVAL_OR, 3}}); sel("underflow not", fs, {NOT});
  sel("bad opcode", fs, {P(0), {9, 0}}); sel("left two", fs, {P(0), P(1)}); sel("drop all", fs, {P(0), {LLKV_EVAL_AND, 1}, P(1)});
  // GatherNullPolicy::DropNulls
  for (auto &drop : std::vector<std::vector<uint32_t>>{{cI64n}, {cI64n, cF64n}, {cI64n, cI64}, {cI64n, cI64n}, {kMissing}, {cI64}, {cI64n, cF64n, cUtfKeyN}})
    for (auto &f : std::vector<std::vector<llkv_filter>>{{}, {fs[0]}, {fs[8]}, {fs[1]}}) sel("dropnull " + std::to_string(drop.size()) + "/" + std::to_string(drop[0]) + " " + std::to_string(f.size() ? f[0].field_id : 0), f, {}, drop);
  // more than 16 column buffers, through each kind of slot
  std::vector<llkv_filter> many;
  for (auto &c : g_cols) if (c.dtype == LLKV_DT_INT64 && c.nullable && many.size() < 9) many.push_back(leaf(c.field_id, LLKV_OP_GT, lit_int(0)));
  sel("18 buffers", many);
  many.pop_back();
  sel("16 buffers", many);
  static const E wide = col(cDecWide), i64n = col(cI64n);
  plan("16 + wide", many, {}, {agg(LLKV_AGG_SUM, 0, &wide)}, 0); plan("16 + wide min", many, {}, {agg(LLKV_AGG_MIN, 0, &wide)}, 0); plan("16 + nullable", many, {}, {agg(LLKV_AGG_SUM, 0, &i64n)}, 0);
  many.pop_back();
  plan("14 + wide", many, {}, {agg(LLKV_AGG_SUM, 0, &wide)}, 0);
  many.push_back(leaf(cI64, LLKV_OP_GT, lit_int(0)));
  plan("15 + wide", many, {}, {agg(LLKV_AGG_SUM, 0, &wide)}, 0); plan("15 + nullable", many, {}, {agg(LLKV_AGG_SUM, 0, &i64n)}, 0); sel("15 + dropnull", many, {}, {cF64n, cI64n});
  // literal banks: 48 integer / float slots
  for (int n_l : {24, 25}) {
    static std::deque<E> keep;
    E sum = col(cI64), fsum = col(cF64);
    for (int i = 0; i < n_l * 2; ++i) { sum = bin(1, sum, lit(lit_int(100 + i), std::to_string(100 + i))); fsum = bin(1, fsum, lit(lit_f64(100.5 + i), "f")); }
    keep.push_back(sum); keep.push_back(fsum);
    const E &s = keep[keep.size() - 2], &f = keep.back();
    for (const E *e : {&s, &f}) { plan("lits " + std::to_string(n_l), {}, {}, {agg(LLKV_AGG_SUM, 0, e)}, 0); plan("lits " + std::to_string(n_l), {}, {cUtfKey}, {agg(LLKV_AGG_SUM, 0, e)}, 1); proj("lits", {{1, 0, e->t.data(), (uint32_t)e->t.size(), nullptr}}, false); }
  }
}

static void aggregates_of(const E &e, int uses) { // uses: 1 ungrouped, 2 grouped, 4 image, 8 reduce, 16 partitioned
  for (int kind = 1; kind <= 9; ++kind)
    for (int distinct = 0; distinct < 2; ++distinct) {
      const std::string nm = "agg k" + std::to_string(kind) + (distinct ? "d " : " ") + e.name;
      const std::vector<llkv_aggregate_spec> a = {agg(kind, distinct, &e)};
      if (uses & 1) plan(nm, {}, {}, a, 0);
      if (uses & 2) plan(nm, {}, {cUtfKey}, a, 1 | (kind & 2));
      if (uses & 4) plan(nm, {}, {cUtfKey}, a, 1 | 4 | (kind & 2));
      if (uses & 16) plan(nm, {}, {cUtfWide}, a, 1 | 4 | 8);
      if (uses & 8) reduce(nm, a);
    }
}

static void section_aggregates(const std::vector<uint32_t> &fields, bool with_exprs) {
  for (uint32_t f : fields) aggregates_of(col(f), 31);
  if (!with_exprs) return;
  for (auto &e : operands_full) aggregates_of(e, 15);
  for (size_t i = 0; i < exprs1.size(); i += g_exact ? 3 : 1) aggregates_of(exprs1[i], 15);
  for (size_t i = 0; i < exprs23.size(); i += g_exact ? 5 : 1) {
    const std::vector<llkv_aggregate_spec> a = {agg(LLKV_AGG_SUM, 0, &exprs23[i])}, d = {agg(LLKV_AGG_SUM, 1, &exprs23[i])}, m = {agg(LLKV_AGG_MIN, 0, &exprs23[i]), agg(LLKV_AGG_AVG, 0, &exprs23[i])};
    plan("agg3 " + exprs23[i].name, {}, {}, a, 0);
    plan("agg3 " + exprs23[i].name, {}, {cUtfKey}, i % 2 ? a : m, 3);
    if (i % 3 == 0) plan("agg3 " + exprs23[i].name, {}, {cUtfKey}, a, 5);
    if (i % 4 == 0) reduce("agg3d " + exprs23[i].name, d);
  }
}

static void section_lists(bool all_flags) {
  static std::vector<E> pool;
  if (pool.empty()) {
    for (uint32_t f : {cI64, cI64n, cI64big, cF64, cF64n, cF64plain, cDec2, cDec0n, cDecWide, cUtfNum, cBoolN}) pool.push_back(col(f));
    const E one = lit(lit_int(1), "1"), d100 = lit(lit_dec(100, 2), "d1.00");
    pool.push_back(bin(3, col(cDec2), bin(2, d100, col(cDec2))));
    pool.push_back(bin(3, col(cDec2), bin(1, d100, col(cDec0n))));
    pool.push_back(bin(1, col(cDec0n), col(cDec0n)));
    pool.push_back(bin(3, col(cDec4), col(cDec2)));
    pool.push_back(bin(1, col(cDec2), d100));
    pool.push_back(bin(2, col(cDec2), d100));
    pool.push_back(bin(4, col(cDec2), d100));
    pool.push_back(bin(3, col(cF64), bin(2, one, col(cF64n))));
    pool.push_back(bin(3, col(cF64), bin(2, one, col(cF64))));
    pool.push_back(bin(1, col(cI64), col(cI64n)));
    pool.push_back(bin(4, col(cI64), col(cI64)));
    for (auto &c : g_cols) if (c.dtype == LLKV_DT_DECIMAL128 && !c.wide128 && c.scale == 2 && c.has_stats && c.min_i == 0) pool.push_back(bin(1, col(c.field_id), d100)); // decimal arguments over tables of 2^38 rows and more
  }
  const int kinds[] = {3, 5, 2, 6, 4, 7, 8, 1, 3, 3};
  std::vector<std::pair<std::string, std::vector<llkv_aggregate_spec>>> lists;
  for (size_t start = 0; start < pool.size(); ++start)
    for (size_t len = 1; len <= 6; ++len)
      for (int rep = 0; rep < 2; ++rep) {
        std::vector<llkv_aggregate_spec> a;
        std::string nm = "list";
        for (size_t i = 0; i < len; ++i) {
          const size_t at = (start + i * (1 + start % 3)) % pool.size();
          const int kind = kinds[(start + i + len) % 10];
          a.push_back(agg(kind, 0, kind == 1 ? nullptr : &pool[at]));
          nm += " " + std::to_string(kind) + ":" + pool[at].name;
        }
        if (rep) { a.push_back(a[0]); a.push_back(agg(LLKV_AGG_AVG, 0, &pool[start])); nm += " +rep"; }
        lists.push_back({nm, a});
      }
  { // every decimal argument at once: FirstDigits packs of four, several validities
    std::vector<llkv_aggregate_spec> a;
    for (auto &e : pool) if (e.name.find("c" + std::to_string(cDec2)) != std::string::npos || e.name.find("c" + std::to_string(cDec0n)) != std::string::npos) a.push_back(agg(LLKV_AGG_SUM, 0, &e));
    lists.push_back({"list all decimals", a});
    a.clear();
    for (size_t i = pool.size() - 6; i < pool.size(); ++i) a.push_back(agg(LLKV_AGG_MAX, 0, &pool[i]));
    lists.push_back({"list big-table decimals", a});
    a.clear();
    for (int i = 0; i < 30; ++i) a.push_back(agg(LLKV_AGG_MIN, 0, &pool[3 + i % 3]));
    for (int i = 0; i < 12; ++i) a.push_back(agg(LLKV_AGG_MAX, 0, &pool[i]));
    lists.push_back({"list many lanes", a});
  }
  const std::vector<llkv_filter> f1 = {leaf(cDate, LLKV_OP_LE, lit_int(10471))};
  for (auto &l : lists) {
    for (int flags : {0, 1, 3, 5, 7, 13, 15}) {
      if (!all_flags && flags != 0 && flags != 3 && flags != 7) continue;
      plan(l.first, flags & 2 ? f1 : std::vector<llkv_filter>{}, flags & 1 ? std::vector<uint32_t>{cUtfKey, cUtfKeyN} : std::vector<uint32_t>{}, l.second, flags);
    }
    if (all_flags) { plan(l.first + " big", {}, {cUtf256, cI64key}, l.second, 5); plan(l.first + " huge", {}, {cUtfWideN, cI64key, cUtfKeyN}, l.second, 5); plan(l.first + " part", {}, {cUtfWide, cUtfKey}, l.second, 15); }
    reduce(l.first, l.second);
    // DISTINCT forms on the sort route: pairs over the same / another argument
    std::vector<llkv_aggregate_spec> d = l.second;
    for (size_t i = 0; i < d.size(); i += 2) d[i].distinct = 1;
    reduce(l.first + " distinct", d);
  }
  // invalid flag combinations, empty lists
  static const E x = col(cI64);
  for (int flags = 0; flags < 16; ++flags) {
    plan("flags", {}, {cUtfKey}, {agg(LLKV_AGG_SUM, 0, &x)}, flags); plan("flags nokeys", {}, {}, {agg(LLKV_AGG_SUM, 0, &x)}, flags); plan("flags noaggs", {}, {cUtfKey}, {}, flags);
    plan("flags false", {leaf(cUtfKey, LLKV_OP_EQUALS, lit_str("zz"))}, {cUtfKey}, {agg(LLKV_AGG_SUM, 0, &x)}, flags);
  }
  reduce("empty", {});
}

static void section_keys() {
  static const E x = col(cI64), fx = col(cF64);
  const std::vector<llkv_aggregate_spec> a = {agg(LLKV_AGG_COUNT_STAR, 0, nullptr), agg(LLKV_AGG_SUM, 0, &x), agg(LLKV_AGG_SUM, 0, &fx)};
  std::vector<uint32_t> K = {cUtfKey, cUtfKeyN, cUtf256, cUtfWide, cUtfWideN, cUtfBig, cI64key, cI64keyN, cI32key, cDateKey, cI64range, cI64ns, cI64big, cF64, cF32, cDec2, cU64, cU32, cBool, cNullT, kMissing};
  for (auto &c : g_cols) if (c.dtype == LLKV_DT_UTF8 && c.dictionary.size() <= 7) K.push_back(c.field_id);
  for (int flags : {1, 3, 5, 7, 13})
    for (uint32_t k1 : K) {
      plan("key " + std::to_string(k1), {}, {k1}, a, flags);
      for (uint32_t k2 : K) if (flags != 13 || (k1 != cUtfBig && k2 != cUtfBig && k1 != cUtfWide)) plan("keys " + std::to_string(k1) + "," + std::to_string(k2), {}, {k1, k2}, a, flags);
    }
  for (int flags : {1, 5, 15}) {
    plan("keys3", {}, {cUtfKey, cI64key, cUtfKeyN}, a, flags); plan("keys4", {}, {cUtfKey, cI64key, cUtfKeyN, cI32key}, a, flags); plan("keys5", {}, {cUtfKey, cI64key, cUtfKeyN, cI32key, cDateKey}, a, flags);
    plan("keys3 big", {}, {cUtf256, cUtf256, cUtf256}, a, flags); plan("keys2 big", {}, {cUtfBig, cUtf256}, a, flags); plan("keys2 wide", {}, {cUtfWide, cUtfWide}, a, flags);
  }
}

static void section_projection(const std::vector<uint32_t> &fields, bool with_exprs) {
  for (int pad = 0; pad < 2; ++pad) {
    for (uint32_t f : fields) {
      const E c = col(f);
      proj("col " + c.name, {{0, f, nullptr, 0, nullptr}}, pad);
      proj("expr " + c.name, {{1, 0, c.t.data(), 1, nullptr}}, pad);
    }
    if (!with_exprs) continue;
    for (auto &e : operands_full) proj("expr " + e.name, {{1, 0, e.t.data(), (uint32_t)e.t.size(), nullptr}}, pad);
    for (size_t i = 0; i < exprs1.size(); i += pad ? 50 : 1) proj("expr " + exprs1[i].name, {{1, 0, exprs1[i].t.data(), (uint32_t)exprs1[i].t.size(), nullptr}}, pad);
    for (size_t i = 0; i < exprs23.size(); i += pad ? 500 : 1) proj("expr " + exprs23[i].name, {{1, 0, exprs23[i].t.data(), (uint32_t)exprs23[i].t.size(), nullptr}}, pad);
    proj("none", {}, pad); proj("null expr", {{1, 0, nullptr, 0, nullptr}}, pad);
    std::vector<llkv_projection> many;
    const std::vector<uint32_t> rf = rep_fields();
    for (size_t i = 0; i < 9; ++i) {
      if (i == 8) proj("eight", many, pad);
      many.push_back({(int32_t)(i % 2 && !pad), rf[i], exprs1[i * 13].t.data(), (uint32_t)exprs1[i * 13].t.size(), nullptr});
    }
    proj("nine", many, pad);
    proj("mixed", {{0, cI64n, nullptr, 0, nullptr}, {0, cDecWide, nullptr, 0, nullptr}, {0, cUtfWideN, nullptr, 0, nullptr}, {0, cI64n, nullptr, 0, nullptr}, {0, cDec0n, nullptr, 0, nullptr}}, pad);
  }
}

static void section_emit_probe(const std::vector<uint32_t> &fields, bool with_exprs) {
  const std::vector<llkv_filter> none, one = {leaf(cDate, LLKV_OP_GT, lit_int(9000))}, never = {leaf(cUtfKey, LLKV_OP_EQUALS, lit_str("zz"))};
  const uint32_t sets[] = {cI64key, cI64keyN, cI32key, cU64, cU32, cDateKey, cF64, cDecWide, cUtfWide, kMissing, cDate};
  for (uint32_t f : fields) {
    for (int flags = 0; flags < 16; ++flags) emit("bare", flags & 4 ? one : none, col(f), flags);
    for (uint32_t s : sets) { emit("set", one, col(f), 3, &s); if (f == cI64) { emit("set", none, col(f), 0, &s); emit("set", never, col(f), 0, &s); } }
    for (auto *fs : {&none, &one, &never}) { in_set("in_set", *fs, f); for (int kb = 0; kb < 2; ++kb) { static const E v = bin(3, col(cF64), bin(2, lit(lit_int(1), "1"), col(cF64ns))); probe("probe", *fs, f, &v, kb); } }
  }
  static const E cf = col(cF64), cdate = col(cDate), ci = col(cI64), cfn = col(cF64n);
  for (int kb = 0; kb < 2; ++kb) { probe("probe", one, cI64key, nullptr, kb); probe("probe", one, cI64key, &cf, kb); probe("probe", one, cI64key, &cdate, kb); probe("probe", none, cI64key, &ci, kb); probe("probe", none, cI64key, &cfn, kb); probe("probe", one, cF64, &cf, kb); }
  if (!with_exprs) return;
  for (auto &e : operands_full) { for (int flags : {0, 1, 3, 15}) emit("expr", none, e, flags); probe("probe", one, cI64key, &e, false); }
  for (size_t i = 0; i < exprs1.size(); ++i) { emit("expr", none, exprs1[i], i % 2 ? 1 : 0); emit("expr", one, exprs1[i], 11, &sets[0]); probe("probe", i % 2 ? one : none, cI32key, &exprs1[i], i % 3 == 0); }
  for (size_t i = 0; i < exprs23.size(); i += 2) { emit("expr", none, exprs23[i], 1); probe("probe", one, cI64key, &exprs23[i + 1], true); }
}

static void section_small_functions() {
  const auto lits = leaf_literals();
  std::vector<llkv_literal> more = lits;
  for (i128 v : {(i128)INT64_MAX, (i128)INT64_MAX + 1, (i128)INT64_MIN, (i128)INT64_MIN - 1, (i128)INT32_MAX, (i128)INT32_MAX + 1, (i128)INT32_MIN - 1, (i128)UINT32_MAX, (i128)UINT32_MAX + 1, (i128)UINT64_MAX, (i128)UINT64_MAX + 1})
    { more.push_back(lit_int(v)); more.push_back(lit_dec(v, 0)); more.push_back(lit_dec(v, 1)); more.push_back(lit_dec(v, -2)); }
  more.push_back(lit_f64(3.5e38)); more.push_back(lit_f64(-INFINITY)); more.push_back(lit_dec(12345, 400)); more.push_back(lit_dec(12345, -400));
  for (int dt = -1; dt <= 11; ++dt)
    for (size_t i = 0; i < more.size(); ++i) {
      NativeLit n; std::string err;
      int rc = cast_literal_for_column(more[i], dt, &n, &err);
      uint64_t fb; memcpy(&fb, &n.f, 8);
      record("cast_literal", "dt" + std::to_string(dt) + " l" + std::to_string(i), rc, err, nullptr, "f=" + std::to_string(n.is_float) + " u=" + std::to_string(n.is_unsigned) + " i=" + std::to_string(n.i) + " fb=" + std::to_string(fb));
    }
  for (auto &c : g_cols) {
    const std::vector<uint32_t> r = dictionary_ranks(c);
    record("dictionary_ranks", "c" + std::to_string(c.field_id), 0, "", nullptr, "n=" + std::to_string(r.size()) + " h=" + std::to_string(fnv(r.data(), r.size() * 4)) + " wide=" + std::to_string(utf8_wide(c)) + " sd=" + std::to_string(storage_dtype(c)));
  }
  for (const char *s : {"", " ", "1", " 2.5 ", "-3e2", "+.5", "5.", ".", "1e", "1e+", "1e+5", "1E-400", "1e400", "0x10", "inf", "-Infinity", "+NaN", "nan", "infinit", "1 2", "\xC2\xA0" "7\xE2\x80\x83", "\xE3\x80\x80", "\t-0.0\n",
                        "12345678901234567890123", "1_0", "--1", "abc", "\xC2\x85" "1.25e2\xE2\x81\x9F", "1d", "1f", "  +inf  "}) {
    const double v = parse_numeric_or_zero(s);
    uint64_t b; memcpy(&b, &v, 8);
    record("parse_numeric", "s" + std::to_string(strlen(s)) + ":" + std::to_string(fnv(s, strlen(s))), 0, "", nullptr, "bits=" + std::to_string(b));
  }
  for (int dt = -1; dt <= 11; ++dt) record("dtype", std::to_string(dt), 0, "", nullptr, std::string(dtype_name(dt)) + " " + dtype_tag(dt) + " " + std::to_string(dtype_width(dt)) + " " + std::to_string(dtype_out_width(dt)));
}

static void run_corpus() {
  section_small_functions();
  section_leaves();
  section_compare();
  section_programs();
  const char *envs[] = {nullptr, "LLKV_HIP_IMAGE_NO_FIXED", "LLKV_HIP_MINMAX_ROW_ORDER", "LLKV_HIP_IMAGE_WIDE_CELLS", "LLKV_HIP_UNROLL", "LLKV_HIP_SCAN_NO_LATE", "LLKV_HIP_JOIN_NO_LATE"};
  for (const char *env : envs)
    for (const char *val : {"1", "8", "3"}) {
      if ((!env || strcmp(env, "LLKV_HIP_UNROLL")) && strcmp(val, "1")) continue;
      if (env) { setenv(env, val, 1); g_env = std::string(env) + "=" + val; }
      for (int exact = 0; exact < 2; ++exact) {
        g_exact = exact;
        plan_set_exact_f64_sums(exact);
        record("option", "exact_f64_sums", 0, "", nullptr, std::to_string(plan_exact_f64_sums()));
        section_aggregates(env ? rep_fields() : all_fields(), !env);
        section_lists(!env || !exact);
        if (!exact) section_keys();
        if (!exact || !env) section_emit_probe(env ? rep_fields() : all_fields(), !env && !exact);
        if (!exact) section_projection(env ? rep_fields() : all_fields(), !env);
      }
      plan_set_exact_f64_sums(false);
      g_exact = false;
      if (env) { unsetenv(env); g_env = "-"; }
    }
}

// ---------------------------------------------------------------- coverage of a plan.cpp by the corpus
static int coverage_report(const char *source, const char *seeds) {
  g_quiet = true;
  run_corpus();
  std::ifstream in(source);
  if (!in) { fprintf(stderr, "cannot read %s\n", source); return 2; }
  std::stringstream ss; ss << in.rdbuf();
  const std::string src = ss.str();
  // string literals of the source, and those that belong to a fail(…) / set_err(…) statement
  std::set<std::string> want_nodes, want_msgs;
  static const std::set<std::string> not_nodes = {"Int64", "Float64", "Int32", "Date32", "UInt64", "UInt32", "Float32", "Utf8", "Boolean", "Decimal128", "Null", "SUM", "TOTAL", "AVG", "MIN", "MAX", "Filtering", "Modulo",
                                                  "LLKV", "Decimal128("};
  size_t stmt_fail_until = 0;
  for (size_t i = 0; i < src.size(); ++i) {
    if (src.compare(i, 2, "//") == 0) { while (i < src.size() && src[i] != '\n') ++i; continue; }
    if (src[i] == '\'') { i += src[i + 1] == '\\' ? 3 : 2; continue; }
    if (src.compare(i, 5, "fail(") == 0 || src.compare(i, 8, "set_err(") == 0) { // to the statement's end
      if (i >= 4 && src.compare(i - 4, 4, "int ") == 0) continue;                     // (their definitions)
      size_t e = i;
      for (bool q = false; e < src.size() && (q || src[e] != ';'); ++e) if (src[e] == '"' && src[e - 1] != '\\') q = !q;
      stmt_fail_until = std::max(stmt_fail_until, e);
    }
    if (src[i] != '"') continue;
    size_t j = i + 1;
    std::string s;
    for (; j < src.size() && src[j] != '"'; ++j) { if (src[j] == '\\') ++j; s += src[j]; }
    if (i < stmt_fail_until) { if (s.size() >= 4) want_msgs.insert(s); }
    else {
      for (size_t a = 0; a < s.size();) {
        if (!isupper((unsigned char)s[a]) || (a && isalnum((unsigned char)s[a - 1]))) { ++a; continue; }
        size_t b = a;
        while (b < s.size() && isalnum((unsigned char)s[b])) ++b;
        if ((b < s.size() && s[b] == '<') || (a == 0 && b == s.size() && b > 2)) want_nodes.insert(s.substr(a, b - a));
        a = b;
      }
    }
    i = j;
  }
  std::ifstream sin(seeds);
  for (std::string line; std::getline(sin, line);) {
    const size_t bar = line.find('|');
    const std::string ts = bar == std::string::npos ? line : line.substr(bar + 1);
    for (size_t a = 0; a < ts.size();) {
      if (!isupper((unsigned char)ts[a])) { ++a; continue; }
      size_t b = a;
      while (b < ts.size() && isalnum((unsigned char)ts[b])) ++b;
      if (b < ts.size() && ts[b] == '<') want_nodes.insert(ts.substr(a, b - a));
      a = b;
    }
  }
  size_t missing = 0;
  printf("records: %zu\n", g_index);
  for (auto &c : g_counts) printf("  %-18s %zu\n", c.first.c_str(), c.second);
  printf("node names wanted: %zu\n", want_nodes.size());
  for (auto &n : want_nodes) {
    if (not_nodes.count(n)) continue;
    const bool hit = g_nodes.count(n);
    if (!hit) { ++missing; printf("  MISSING node %s\n", n.c_str()); }
  }
  printf("node names reached:");
  for (auto &n : want_nodes) if (g_nodes.count(n)) printf(" %s", n.c_str());
  printf("\nfail()/set_err() message literals wanted: %zu, distinct error texts produced: %zu\n", want_msgs.size(), g_errs.size());
  for (auto &m : want_msgs) {
    bool hit = false;
    for (auto &e : g_errs) if (e.find(m) != std::string::npos) { hit = true; break; }
    if (!hit) { ++missing; printf("  MISSING message \"%s\"\n", m.c_str()); }
  }
  printf("missing: %zu\n", missing);
  return 0;
}

// ---------------------------------------------------------------- host time of representative lowerings
static int time_mode() {
  g_quiet = true;
  auto mkc = [&](int32_t dt, uint64_t rows) { ColumnInfo c; c.dtype = dt; c.rows = rows; return c; };
  const uint64_t N = 59986052;
  auto f64c = [&](double mx, double mn) { ColumnInfo c = mkc(LLKV_DT_FLOAT64, N); c.has_fstats = c.f_all_finite = c.f_no_nan = c.f_no_neg_zero = true; c.f_absmax = mx; c.f_absmin_nz = mn; return add_col(c); };
  const uint32_t qty = f64c(50, 1), price = f64c(104949.5, 900.0), disc = f64c(0.1, 0.01), tax = f64c(0.08, 0.01);
  ColumnInfo c = mkc(LLKV_DT_UTF8, N); c.dictionary = {"A", "N", "R"}; const uint32_t rf = add_col(c); c.dictionary = {"F", "O"}; const uint32_t ls = add_col(c);
  c = mkc(LLKV_DT_DATE32, N); c.has_stats = true; c.min_i = 8035; c.max_i = 10561; const uint32_t ship = add_col(c);
  c = mkc(LLKV_DT_INT64, N); c.has_stats = true; c.min_i = 1; c.max_i = 60000000; const uint32_t okey = add_col(c);
  c = mkc(LLKV_DT_INT32, 15000000); c.has_stats = true; c.min_i = 1; c.max_i = 1500000; const uint32_t ckey = add_col(c);
  c = mkc(LLKV_DT_DATE32, 15000000); c.has_stats = true; c.min_i = 8035; c.max_i = 10440; const uint32_t odate = add_col(c);
  c = mkc(LLKV_DT_DECIMAL128, N); c.precision = 15; c.scale = 2; c.has_stats = true; c.min_i = 0; c.max_i = 10494950; const uint32_t dprice = add_col(c); c.max_i = 10; const uint32_t ddisc = add_col(c);
  const E one = lit(lit_int(1), "1"), d1 = lit(lit_dec(100, 2), "1.00");
  const E rev = bin(3, col(price), bin(2, one, col(disc))), charge = bin(3, rev, bin(1, one, col(tax))), q6 = bin(3, col(price), col(disc)), cq = col(qty), cp = col(price), cd = col(disc), cok = col(okey);
  const E drev = bin(3, col(dprice), bin(2, d1, col(ddisc))), dsum = bin(1, col(dprice), col(ddisc)), dp = col(dprice), dd = col(ddisc);
  const std::vector<llkv_aggregate_spec> q1 = {agg(3, 0, &cq), agg(3, 0, &cp), agg(3, 0, &rev), agg(3, 0, &charge), agg(5, 0, &cq), agg(5, 0, &cp), agg(5, 0, &cd), agg(1, 0, nullptr)};
  const std::vector<llkv_aggregate_spec> dec6 = {agg(3, 0, &drev), agg(5, 0, &drev), agg(3, 0, &dsum), agg(6, 0, &dp), agg(7, 0, &dd), agg(3, 0, &dp)};
  llkv_filter r1 = leaf(ship, LLKV_OP_RANGE); r1.lower_kind = 1; r1.lower = lit_int(8766); r1.upper_kind = 2; r1.upper = lit_int(9131);
  llkv_filter r2 = leaf(disc, LLKV_OP_RANGE); r2.lower_kind = 1; r2.lower = lit_f64(0.05); r2.upper_kind = 1; r2.upper = lit_f64(0.07);
  llkv_filter pat = leaf(cUtfWide, LLKV_OP_CONTAINS, lit_str("K15")); pat.case_sensitive = 0;
  struct Case { const char *name; std::function<void()> run; };
  const std::vector<Case> cases = {
      {"q1", [&] { plan("t", {leaf(ship, LLKV_OP_LE, lit_int(10471))}, {rf, ls}, q1, 1); }},
      {"q6", [&] { plan("t", {r1, r2, leaf(qty, LLKV_OP_LT, lit_f64(24))}, {}, {agg(3, 0, &q6)}, 0); }},
      {"q3_probe", [&] { probe("t", {leaf(ship, LLKV_OP_GT, lit_int(9204))}, okey, &rev, false); }},
      {"q3_emit_orders", [&] { emit("t", {leaf(odate, LLKV_OP_LT, lit_int(9204))}, col(ckey), 2, &ckey); }},
      {"q3_emit_keybits", [&] { emit("t", {leaf(ship, LLKV_OP_GT, lit_int(9204))}, cok, 2 | 4, &okey); }},
      {"decimal_groupby6", [&] { plan("t", {leaf(ship, LLKV_OP_LE, lit_int(10471))}, {rf, ls}, dec6, 3); }},
      {"wide_utf8_pattern", [&] { sel("t", {pat}); }}};
  for (auto &cs : cases) {
    std::vector<double> runs;
    for (int r = 0; r < 15; ++r) {
      const int reps = 2000;
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; i < reps; ++i) cs.run();
      runs.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps);
    }
    std::sort(runs.begin(), runs.end());
    printf("%-18s median_us %.3f min_us %.3f max_us %.3f\n", cs.name, runs[7], runs[0], runs[14]);
  }
  return 0;
}

int main(int argc, char **argv) {
  for (const char *env : {"LLKV_HIP_IMAGE_NO_FIXED", "LLKV_HIP_MINMAX_ROW_ORDER", "LLKV_HIP_IMAGE_WIDE_CELLS", "LLKV_HIP_UNROLL", "LLKV_HIP_SCAN_NO_LATE", "LLKV_HIP_JOIN_NO_LATE"}) unsetenv(env);
  build_catalogue();
  build_expressions();
  if (argc >= 4 && !strcmp(argv[1], "--coverage-report")) return coverage_report(argv[2], argv[3]);
  if (argc >= 2 && !strcmp(argv[1], "--time")) return time_mode();
  run_corpus();
  for (auto &c : g_counts) fprintf(stderr, "%-18s %zu\n", c.first.c_str(), c.second);
  fprintf(stderr, "records %zu\n", g_index);
  return 0;
}
