// group_cell.hip.h — the device restatement of finalize_value (engine.cpp): one aggregate's finalized cell from a group's lanes,
// bit for bit what the host returns, and the check of the aggregates whose finalize can fail.  Included by the device top-k
// (group_order.hip: order images of the cells) and the device HAVING (group_having.hip: the cells themselves).
#pragma once
#include "engine.hpp"

namespace llkv {
namespace {

typedef __int128 i128;
typedef unsigned __int128 u128;

constexpr int kMaxErrAggs = 16; // aggregates whose finalize can fail

// What agg_cell needs of an AggOut (plan.hpp), as plain kernel-argument data.
struct AggCell {
  int32_t fin;              // AggFinal
  int32_t lane, count_lane; // relative to the group's aggregate lanes (after rows and first row id)
  int32_t typed_by_first_value, fast_sum, wide, plain_minmax, null_without_values, fixed_point, fixed_exp, exact_levels, wide_delta, nan_default;
  uint64_t wide_base_hi, wide_base_lo;
};

inline void agg_cell_of(const AggOut &a, AggCell *t) {
  t->fin = (int32_t)a.fin;
  t->lane = a.lane;
  t->count_lane = a.count_lane;
  t->typed_by_first_value = a.typed_by_first_value;
  t->fast_sum = a.fast_sum;
  t->wide = a.wide;
  t->plain_minmax = a.plain_minmax;
  t->null_without_values = a.null_without_values;
  t->fixed_point = a.fixed_point;
  t->fixed_exp = a.fixed_exp;
  t->exact_levels = a.exact_levels;
  t->wide_delta = a.wide_delta;
  t->nan_default = a.nan_default;
  t->wide_base_hi = a.wide_base_hi;
  t->wide_base_lo = a.wide_base_lo;
}

enum AggCellType : int32_t { kCellI64 = 0, kCellF64 = 1, kCellDec = 2 }; // of a non-NULL cell
__host__ __device__ inline int32_t agg_cell_type(AggFinal f) {
  switch (f) {
  case AggFinal::SumDec: case AggFinal::TotalDec: case AggFinal::AvgDec: case AggFinal::MinDec: case AggFinal::MaxDec: return kCellDec;
  case AggFinal::SumF64: case AggFinal::TotalF64: case AggFinal::AvgI64: case AggFinal::AvgI64Fast: case AggFinal::AvgF64: case AggFinal::MinF64: case AggFinal::MaxF64:
    return kCellF64;
  default: return kCellI64;
  }
}
inline bool agg_finalize_can_fail(AggFinal f) { return f == AggFinal::SumI64 || f == AggFinal::AvgI64; }

__device__ inline double as_f64(uint64_t b) { return __longlong_as_double((long long)b); }
__device__ inline uint64_t as_u64(double d) { return (uint64_t)__double_as_longlong(d); }

// The host's (x86-64 SSE2) NaN results, so that a NaN orders where the host's would: an operand NaN comes back quieted, the
// first one first; an invalid operation yields the default NaN, sign bit set.
constexpr uint64_t kQuiet = 0x0008000000000000ull;
__device__ inline double host_add(double a, double b) {
  if (__builtin_isnan(a)) return as_f64(as_u64(a) | kQuiet);
  if (__builtin_isnan(b)) return as_f64(as_u64(b) | kQuiet);
  const double r = a + b;
  return __builtin_isnan(r) ? as_f64(0xFFF8000000000000ull) : r;
}
__device__ inline double host_div_rows(double a, int64_t rows) { // rows > 0
  if (__builtin_isnan(a)) return as_f64(as_u64(a) | kQuiet);
  return a / (double)rows;
}

// (double) of an i128, rounded to nearest even like the host's conversion
__device__ inline double i128_to_f64(i128 v) {
  const bool neg = v < 0;
  const u128 m = neg ? (u128)0 - (u128)v : (u128)v;
  const uint64_t hi = (uint64_t)(m >> 64), lo = (uint64_t)m;
  if (!hi && !(lo >> 53)) { const double r = (double)lo; return neg ? -r : r; } // exact
  const int msb = hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);
  const int sh = msb - 52; // keep 53 bits
  u128 q = m >> sh;
  const u128 rem = m & (((u128)1 << sh) - 1), half = (u128)1 << (sh - 1);
  if (rem > half || (rem == half && (q & 1))) q += 1; // (a carry to 2^53 is still exact)
  const double r = ldexp((double)(uint64_t)q, sh);
  return neg ? -r : r;
}

// |m| / d and its remainder (d > 0): AVG over Decimal128
__device__ inline void udiv128(u128 m, uint64_t d, u128 *q, uint64_t *r) {
  if (!(uint64_t)(m >> 64)) { *q = (uint64_t)m / d; *r = (uint64_t)m % d; return; }
  u128 quo = 0, rem = 0;
  for (int i = 127; i >= 0; --i) {
    rem = (rem << 1) | ((m >> i) & 1);
    if (rem >= d) { rem -= d; quo |= (u128)1 << i; }
  }
  *q = quo;
  *r = (uint64_t)rem;
}

__device__ inline i128 exact_total(const uint64_t *l) { return ((i128)(int64_t)l[1] << 32) + (i128)(u128)l[0]; }

// SUM / AVG over i64 (agg_finalize_can_fail): the total outside i64, or a prefix that may have left it — finalize_value's exact_sum
__device__ inline bool agg_finalize_fails(const uint64_t *g, int32_t lane, int32_t count_lane) {
  const int64_t rows = count_lane >= 0 ? (int64_t)g[2 + count_lane] : (int64_t)g[0];
  if (rows == 0) return false;
  const uint64_t *l = g + 2 + lane;
  const i128 total = exact_total(l);
  return total > (i128)INT64_MAX || total < (i128)INT64_MIN || __umul64hi(l[2], (uint64_t)rows) != 0 || l[2] * (uint64_t)rows > (uint64_t)INT64_MAX;
}

// finalize_value (engine.cpp) of one aggregate, on the device: *null, or the finalized cell — *c0 = the i64, the f64's bits or the
// high word of a Decimal128 (agg_cell_type says which), *c1 = the Decimal128's low word.  THE device restatement of the host
// finalize: the order images (group_order.hip) and the HAVING cells (group_having.hip) are both made from it.
__device__ inline void agg_cell(const AggCell &t, const uint64_t *g, bool *null, uint64_t *c0, uint64_t *c1) {
  const int64_t rows = t.count_lane >= 0 ? (int64_t)g[2 + t.count_lane] : (int64_t)g[0];
  const uint64_t *l = g + 2 + (t.lane >= 0 ? t.lane : 0);
  const AggFinal fin = (AggFinal)t.fin;
  *null = false;
  *c0 = *c1 = 0;
  if (t.typed_by_first_value && rows == 0 &&
      (fin == AggFinal::SumF64 || fin == AggFinal::MinF64 || fin == AggFinal::MaxF64 || fin == AggFinal::SumDec || fin == AggFinal::MinDec || fin == AggFinal::MaxDec)) {
    *null = true;
    return;
  }
  auto f64_sum = [&]() -> double {
    if (t.fixed_point) return ldexp(i128_to_f64(exact_total(l)), t.fixed_exp);
    double v = as_f64(l[t.exact_levels <= 1 ? 0 : t.exact_levels - 1]);
    for (int j = t.exact_levels - 2; j >= 0; --j) v = host_add(v, as_f64(l[j]));
    return t.nan_default && __builtin_isnan(v) ? as_f64(0xFFF8000000000000ull) : v; // (AggOut::nan_default)
  };
  auto dec = [&](i128 v) {
    *c0 = (uint64_t)(v >> 64);
    *c1 = (uint64_t)v;
  };
  switch (fin) {
  case AggFinal::MinDec: case AggFinal::MaxDec: {
    if (rows == 0) { *null = true; return; }
    if (t.wide_delta) {
      const i128 base = (i128)(((u128)t.wide_base_hi << 64) | t.wide_base_lo);
      dec(t.wide_delta == 1 ? base + (i128)(u128)l[0] : base - (i128)(u128)l[0]);
    } else dec((i128)(int64_t)l[0]);
    return;
  }
  case AggFinal::SumDec: case AggFinal::TotalDec: case AggFinal::AvgDec: {
    const i128 sum = t.wide ? (i128)((u128)l[0] + ((u128)l[1] << 32) + ((u128)l[2] << 64) + ((u128)l[3] << 96))
                            : t.fast_sum ? (i128)(int64_t)l[0] : exact_total(l);
    if (fin == AggFinal::AvgDec) {
      if (rows <= 0) { *null = true; return; }
      const bool neg = sum < 0;
      u128 q;
      uint64_t r;
      udiv128(neg ? (u128)0 - (u128)sum : (u128)sum, (uint64_t)rows, &q, &r);
      i128 v = neg ? -(i128)q : (i128)q;
      if ((u128)r * 2 >= (u128)(uint64_t)rows) v += neg ? -1 : 1; // half away from zero
      dec(v);
      return;
    }
    if (t.null_without_values && rows == 0) { *null = true; return; }
    dec(sum);
    return;
  }
  case AggFinal::CountRows: *c0 = (uint64_t)(rows); return;
  case AggFinal::CountNullsZero: *c0 = (uint64_t)(0); return;
  case AggFinal::CountValid: *c0 = (uint64_t)((int64_t)l[0]); return;
  case AggFinal::CountNulls: *c0 = (uint64_t)((int64_t)g[0] - (int64_t)l[0]); return;
  case AggFinal::SumI64Fast: case AggFinal::MinI64: case AggFinal::MaxI64:
    if (rows == 0) { *null = true; return; }
    *c0 = (uint64_t)((int64_t)l[0]);
    return;
  case AggFinal::SumI64:
    if (rows == 0) { *null = true; return; }
    *c0 = (uint64_t)((int64_t)exact_total(l)); // (a total outside i64 fails the query: agg_finalize_fails)
    return;
  case AggFinal::SumF64: if (rows == 0) { *null = true; return; } *c0 = as_u64(f64_sum()); return;
  case AggFinal::TotalF64: *c0 = as_u64(f64_sum()); return;
  case AggFinal::AvgI64Fast:
    if (rows == 0) { *null = true; return; }
    *c0 = as_u64((double)(int64_t)l[0] / (double)rows);
    return;
  case AggFinal::AvgI64:
    if (rows == 0) { *null = true; return; }
    *c0 = as_u64((double)(int64_t)exact_total(l) / (double)rows);
    return;
  case AggFinal::AvgF64: if (rows == 0) { *null = true; return; } *c0 = as_u64(host_div_rows(f64_sum(), rows)); return;
  case AggFinal::MinF64: case AggFinal::MaxF64: {
    if (rows == 0) { *null = true; return; }
    const uint64_t nan = 0x7FF8000000000000ull; // std::nan("")
    auto key_to_f64 = [](int64_t key) { return (uint64_t)(key < 0 ? (key ^ 0x7FFFFFFFFFFFFFFFll) : key); };
    if (t.plain_minmax) { *c0 = key_to_f64((int64_t)l[0]); return; }
    if (l[2] & 1u) { *c0 = nan; return; }
    const uint64_t none = fin == AggFinal::MinF64 ? 0x7FFFFFFFFFFFFFFFull : 0x8000000000000000ull;
    if (l[0] == none) { *c0 = nan; return; }
    uint64_t v = key_to_f64((int64_t)l[0]);
    if (as_f64(v) == 0.0 && l[1] != 0x7FFFFFFFFFFFFFFFull && (l[1] & 1u)) v = 0x8000000000000000ull; // −0.0
    *c0 = v;
    return;
  }
  }
}

} // namespace
} // namespace llkv
