// having_rules.h — the numeric rules of HAVING (evaluate_having_expr llkv-executor/src/lib.rs:6667-7006), written once for the host
// evaluator (having.cpp) and the device flag kernel (group_having.hip).  Strings exist on the host only: they never compare TRUE
// (:6790) and match only other strings in an IN list (:6849), which having.cpp adds on top of in_match().
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LLKV_HD __host__ __device__
#else
#define LLKV_HD
#endif

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

LLKV_HD inline int32_t having_not(int32_t t) { return t == kHavingNull ? kHavingNull : t == kHavingTrue ? kHavingFalse : kHavingTrue; }

} // namespace llkv
