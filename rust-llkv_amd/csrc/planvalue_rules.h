// planvalue_rules.h — the per-row rules of conditional expressions inside GROUP BY aggregate arguments (ScalarExpr::{Compare, Not,
// IsNull, Cast, Case, Coalesce} and the logical And / Or as evaluate_expr_with_plan_value_aggregates_and_row evaluates them,
// llkv-executor/src/lib.rs:7008-7632, :10035-10084), written once for the device nodes (fused_scan.hip.h: CmpPV … CoalescePV) and
// the host evaluator (planvalue_eval.cpp: llkv_hip_scalar_eval_planvalue).  Scalars in, scalars out: the device knows the class
// of every value from its node type, the host from a tag, and both come here for what the value is.  Strings exist on the host
// only (the device sees a 256-bit code mask the lowering built with pv_compare_bytes' verdicts); nothing here can fail, and
// nothing here reads or writes memory.  Part of the source hiprtc compiles: no header but scan_params.h.
#pragma once
#include "scan_params.h"

#define LLKV_PV_INLINE LLKV_HOST_DEVICE __attribute__((always_inline)) inline

namespace llkv {

// the class of a value; Null is a class of its own only for the NULL literal
enum PvClass : int { kPvNull = 0, kPvInteger = 1, kPvFloat = 2, kPvString = 3, kPvDate32 = 4, kPvDecimal = 5 };

// Rust's `f64 as i64`: saturating, NaN → 0 (spelled out: the C++ conversion of an out-of-range value is undefined)
LLKV_PV_INLINE int64_t pv_f64_as_i64(double x) {
  if (x != x) return 0;
  if (x >= 9223372036854775808.0) return 0x7FFFFFFFFFFFFFFFll;
  if (x <= -9223372036854775808.0) return (int64_t)0x8000000000000000ull;
  return (int64_t)x;
}

// llkv_compare_op over the native operators of T: IEEE for f64 (a NaN operand: only != holds); op 0: the pairing of classes
// does not compare by value (`_ => false`, :7139)
template <class T> LLKV_PV_INLINE bool pv_rel(int op, T a, T b) {
  return op == 1 ? a == b : op == 2 ? a != b : op == 3 ? a < b : op == 4 ? a <= b : op == 5 ? a > b : op == 6 ? a >= b : false;
}
// COMPARE (:7045-7140) over two non-Null values: Int / Int natively, anything with a Float through f64 (the integer `as f64`)
LLKV_PV_INLINE bool pv_compare(int op, int64_t a, int64_t b) { return pv_rel<int64_t>(op, a, b); }
LLKV_PV_INLINE bool pv_compare(int op, double a, double b) { return pv_rel<double>(op, a, b); }
LLKV_PV_INLINE bool pv_compare(int op, int64_t a, double b) { return pv_rel<double>(op, (double)a, b); }
LLKV_PV_INLINE bool pv_compare(int op, double a, int64_t b) { return pv_rel<double>(op, a, (double)b); }
// … String / String by bytes: `order` is the sign of the byte-wise comparison (memcmp, then the lengths)
LLKV_PV_INLINE bool pv_compare_bytes(int op, int order) { return pv_rel<int>(op, order, 0); }
// the pairings that compare by value; every other pairing of two non-Null values is Integer 0 (Date32 against Date32 too)
LLKV_PV_INLINE bool pv_comparable(int l, int r) {
  const bool ln = l == kPvInteger || l == kPvFloat, rn = r == kPvInteger || r == kPvFloat;
  return (ln && rn) || (l == kPvString && r == kPvString);
}

// the truth of a non-Null Integer / Float: NOT (:7141-7157), AND / OR (:10035-10084), a searched CASE's WHEN (:7548-7563; a NaN is true)
LLKV_PV_INLINE bool pv_truth(int64_t v) { return v != 0; }
LLKV_PV_INLINE bool pv_truth(double v) { return v != 0.0; }
LLKV_PV_INLINE int64_t pv_not(bool truth) { return truth ? 0 : 1; }

// three-valued AND / OR: (truth, known) of both sides → the result's truth, and whether it is known (unknown = Null)
LLKV_PV_INLINE bool pv_and(bool lt, bool lk, bool rt, bool rk, bool *known) {
  const bool some_false = (lk & !lt) | (rk & !rt);
  *known = some_false | (lk & rk);
  return !some_false;
}
LLKV_PV_INLINE bool pv_or(bool lt, bool lk, bool rt, bool rk, bool *known) {
  const bool some_true = (lk & lt) | (rk & rt);
  *known = some_true | (lk & rk);
  return some_true;
}

// CAST (:7433-7516) of a non-Null value; the 32-bit targets are not narrowed
LLKV_PV_INLINE int64_t pv_cast_i64(int64_t v) { return v; }
LLKV_PV_INLINE int64_t pv_cast_i64(double v) { return pv_f64_as_i64(v); }
LLKV_PV_INLINE double pv_cast_f64(int64_t v) { return (double)v; }
LLKV_PV_INLINE double pv_cast_f64(double v) { return v; }

// caps of a program (include/llkv_hip.h: LLKV_COND_MAX_*)
constexpr uint32_t kCondMaxTokens = 64, kCondMaxWhens = 8, kCondMaxItems = 8;

} // namespace llkv
