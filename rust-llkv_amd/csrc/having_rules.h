// having_rules.h — the numeric rules of HAVING (evaluate_having_expr llkv-executor/src/lib.rs:6667-7006; value expressions as
// operands: evaluate_expr_with_plan_value_aggregates_and_row :7177-7516), written once for the host
// evaluator (having.cpp) and the device flag kernel (group_having.hip).  Strings exist on the host only: they never compare TRUE
// (:6790) and match only other strings in an IN list (:6849), which having.cpp adds on top of in_match().
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LLKV_HD __host__ __device__
#else
#define LLKV_HD
#endif
#define LLKV_HD_INLINE LLKV_HD __attribute__((always_inline)) inline

namespace llkv {

enum HavingTruth : int32_t { kHavingNull = -1, kHavingFalse = 0, kHavingTrue = 1 };

// PlanValue of a cell or literal.  Integer / Float carry `bits`; the rest are told apart only because no rule looks inside them.
enum HavingTag : int32_t { kHvNull = 0, kHvInteger = 1, kHvFloat = 2, kHvString = 3, kHvDecimal = 4, kHvDate32 = 5 };
struct HavingValue {
  int32_t tag;
  uint64_t bits; // Integer: the i64; Float: the f64's bits
};

LLKV_HD inline double having_f64(const HavingValue &v) {
  if (v.tag == kHvInteger) return (double)(int64_t)v.bits; // `as f64`: round to nearest even
  double d;
  __builtin_memcpy(&d, &v.bits, 8);
  return d;
}

template <class T> LLKV_HD inline bool having_cmp(int32_t op, T l, T r) { // llkv_compare_op; the operators of the type (IEEE for f64)
  switch (op) {
  case 1: return l == r;
  case 2: return l != r;
  case 3: return l < r;
  case 4: return l <= r;
  case 5: return l > r;
  default: return l >= r;
  }
}

// :6716-6791
LLKV_HD inline int32_t having_compare(int32_t op, const HavingValue &l, const HavingValue &r) {
  if (l.tag == kHvNull || r.tag == kHvNull) return kHavingNull;
  const bool li = l.tag == kHvInteger, ri = r.tag == kHvInteger, lf = l.tag == kHvFloat, rf = r.tag == kHvFloat;
  if (li && ri) return having_cmp<int64_t>(op, (int64_t)l.bits, (int64_t)r.bits);
  if ((li || lf) && (ri || rf)) return having_cmp<double>(op, having_f64(l), having_f64(r));
  return kHavingFalse;
}

// one item of an IN list against the (non-Null) test value, numeric pairings (:6844-6848)
LLKV_HD inline bool having_in_match(const HavingValue &t, const HavingValue &item) {
  const bool ti = t.tag == kHvInteger, ii = item.tag == kHvInteger, tf = t.tag == kHvFloat, itf = item.tag == kHvFloat;
  if (ti && ii) return t.bits == item.bits;
  if ((ti || tf) && (ii || itf)) return having_f64(t) == having_f64(item);
  return false;
}

LLKV_HD inline int32_t having_in_result(bool found, bool has_null, bool negated) { // :6865-6883
  if (found) return negated ? kHavingFalse : kHavingTrue;
  if (has_null) return kHavingNull;
  return negated ? kHavingTrue : kHavingFalse;
}

// The truth stack as two bit stacks (bit 0 = top): no array, so the device thread keeps it in two registers.  AND / OR over the
// top n values (:6902-6937; nothing in scope can fail, so the short circuit only decides the value).
struct HavingStack {
  uint64_t val = 0, null = 0;
  LLKV_HD void push(int32_t t) {
    val = (val << 1) | (t == kHavingTrue ? 1u : 0u);
    null = (null << 1) | (t == kHavingNull ? 1u : 0u);
  }
  LLKV_HD int32_t pop() {
    const int32_t t = (null & 1u) ? kHavingNull : (val & 1u) ? kHavingTrue : kHavingFalse;
    val >>= 1;
    null >>= 1;
    return t;
  }
  LLKV_HD int32_t pop_and(uint32_t n) { // n in 1 … 63
    const uint64_t m = (1ull << n) - 1, v = val & m, u = null & m;
    val >>= n;
    null >>= n;
    return (~v & ~u & m) ? kHavingFalse : u ? kHavingNull : kHavingTrue;
  }
  LLKV_HD int32_t pop_or(uint32_t n) {
    const uint64_t m = (1ull << n) - 1, v = val & m, u = null & m;
    val >>= n;
    null >>= n;
    return (v & ~u) ? kHavingTrue : u ? kHavingNull : kHavingFalse;
  }
};
constexpr uint32_t kHavingMaxDepth = 63; // of the bit stacks: a deeper program is refused (host and device alike)

// ---- value expressions as operands (:7177-7516): Null / Integer / Float only — the callers refuse every other leaf ----
// No mul + add pair may be contracted into an fma (hipcc contracts device code by default): having_arith, the one rule that does
// f64 arithmetic, does ONE operation per call and turns contraction off for its own body — its instructions keep that wherever
// the function is inlined, and nothing else in a translation unit that includes this header changes its mode.

constexpr uint32_t kHavingMaxValueDepth = 8; // LLKV_HAVING_MAX_VALUE_DEPTH: pending values of one expression (host and device alike)

LLKV_HD inline HavingValue having_float(double d) {
  HavingValue v{kHvFloat, 0};
  __builtin_memcpy(&v.bits, &d, 8);
  return v;
}

// Rust's `f64 as i64`: saturating, NaN → 0 (spelled out: the C++ conversion of an out-of-range value is undefined)
LLKV_HD inline int64_t having_sat_i64(double d) {
  if (d != d) return 0;
  if (d >= 9223372036854775808.0) return INT64_MAX;
  if (d <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)d;
}
LLKV_HD inline int64_t having_as_i64(const HavingValue &v) { return v.tag == kHvInteger ? (int64_t)v.bits : having_sat_i64(having_f64(v)); }

// ADD SUB MUL DIV MOD (:7194-7390); op: llkv_having_token_op
LLKV_HD inline HavingValue having_arith(int32_t op, const HavingValue &l, const HavingValue &r) {
#pragma clang fp contract(off)
  if (l.tag == kHvNull || r.tag == kHvNull) return {kHvNull, 0};
  const bool ints = l.tag == kHvInteger && r.tag == kHvInteger;
  if (op == 5 && ints) { // DIV, Integer / Integer
    const int64_t a = (int64_t)l.bits, b = (int64_t)r.bits;
    if (b == 0) return {kHvNull, 0};
    if (a == INT64_MIN && b == -1) return having_float((double)a / (double)b);
    return {kHvInteger, (uint64_t)(a / b)};
  }
  const double a = having_f64(l), b = having_f64(r);
  double x;
  switch (op) {
  case 2: x = a + b; break;
  case 3: x = a - b; break;
  case 4: x = a * b; break;
  case 5:
    if (b == 0.0) return {kHvNull, 0};
    x = a / b; // IEEE division
    return having_float(x);
  default: // MOD: Rust's % on f64 = fmod, the sign of the dividend
    if (b == 0.0) return {kHvNull, 0};
    x = ::fmod(a, b);
    break;
  }
  if (!ints) return having_float(x);
  return {kHvInteger, (uint64_t)having_sat_i64(x)};
}

// SHL SHR (:7393-7430): wrapping_shl / wrapping_shr(rhs as u32) — the low 6 bits of the count; SHR arithmetic
LLKV_HD inline HavingValue having_shift(int32_t op, const HavingValue &l, const HavingValue &r) {
  if (l.tag == kHvNull || r.tag == kHvNull) return {kHvNull, 0};
  const int64_t a = having_as_i64(l);
  const uint32_t n = (uint32_t)(uint64_t)having_as_i64(r) & 63u;
  if (op == 7) return {kHvInteger, (uint64_t)a << n};
  return {kHvInteger, (uint64_t)(a >> n)};
}

// CAST to an integer / float type (:7433-7480)
LLKV_HD inline HavingValue having_cast(int32_t op, const HavingValue &v) {
  if (v.tag == kHvNull) return {kHvNull, 0};
  if (op == 9) return {kHvInteger, (uint64_t)having_as_i64(v)};
  return having_float(having_f64(v));
}

// The value stack of one expression, at most kHavingMaxValueDepth deep: named slots and rotate-on-push, never an indexed
// array, so the device thread keeps it in registers (no scratch; always inlined, so that the slots are plain values in the
// kernel).  s0 is the top.
struct HavingValueStack {
  HavingValue s0{0, 0}, s1{0, 0}, s2{0, 0}, s3{0, 0}, s4{0, 0}, s5{0, 0}, s6{0, 0}, s7{0, 0};
  LLKV_HD_INLINE void push(const HavingValue &v) {
    s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0;
    s0 = v;
  }
  LLKV_HD_INLINE HavingValue pop() {
    const HavingValue v = s0;
    s0 = s1; s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
    return v;
  }
};

// One non-PUSH token of a validated expression over the stack; op: llkv_having_token_op.
LLKV_HD_INLINE void having_token(HavingValueStack &st, int32_t op, uint32_t arg) {
  if (op == 11) { // COALESCE: the values come off last first, so the first non-Null in source order is the last one popped
    HavingValue out{kHvNull, 0};
    for (uint32_t i = 0; i < arg; ++i) {
      const HavingValue v = st.pop();
      if (v.tag != kHvNull) out = v;
    }
    st.push(out);
    return;
  }
  if (op == 9 || op == 10) { st.push(having_cast(op, st.pop())); return; }
  const HavingValue r = st.pop(), l = st.pop();
  st.push(op >= 7 ? having_shift(op, l, r) : having_arith(op, l, r));
}

LLKV_HD inline int32_t having_not(int32_t t) { return t == kHavingNull ? kHavingNull : t == kHavingTrue ? kHavingFalse : kHavingTrue; }

} // namespace llkv
