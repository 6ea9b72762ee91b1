// aggregate_column.hip — aggregate columns (include/llkv_hip.h: llkv_hip_table_add_aggregate_columns).
//
// An aggregate column is a column of the OUTER table that holds, for every outer row, the single cell of the reference's correlated
// scalar subquery  SELECT agg(x) FROM inner WHERE <filters> AND inner.key = outer.key[r]  (evaluate_scalar_subquery_with_bindings
// llkv-executor/src/lib.rs:788-834, one execution per distinct binding :836-961): the ungrouped aggregate over the qualifying inner
// rows with that key, the empty set included (COUNT 0, TOTAL 0.0, a decimal SUM 0, every other kind NULL).  It is made in HBM and
// registered like a join column (join_column.hip), whose lifetime rules it shares.
//   accumulate  one thread per qualifying inner row (the selection of inner's filters, ascending rows): d = key − min, then one
//               non-returning device-scope atomic per lane into state[lane][d] — add for the counts and the integer / decimal sums
//               (wrapping; the host excluded overflow by the statistics), min / max on an order-preserving u64 image.  A wave in
//               which neighbouring rows share a key (a clustered key, or one hot key) first reduces every run of equal neighbours
//               with shuffles and sends one atomic per run; skew costs time, never correctness.  The same pass writes d as the
//               sort key of the row when an f64 sum is asked for (a NULL key: span + 1, behind every real key).
//   f64 sums    SUM / AVG / TOTAL accumulate in f64 in row order (llkv-aggregate update: strictly sequential, arrival order), so
//               their bits depend on the order: a stable radix sort of (d, device row) over the bits of span + 1 keeps the rows of a
//               key in ascending table order, and the head of every run of equal keys walks its run and adds left to right, for
//               every f64 lane at once.  One lane per run, however long: no float atomics, the same bits on every run and geometry.
//   finalise    one thread per key: lanes → one 8-byte cell image and one validity byte per requested column
//   lookup      join_lookup_kernel's shape over the outer image: persistent grid, 4 rows per lane, keys as 16-byte loads, the cells
//               gathered at d, one vector store pair per column and one word of validity, padding rows written as NULL cells,
//               counts per wave, then per workgroup, then one atomic per counter.  A NULL or out-of-range key gets the column's
//               empty-set cell.
// LDS: 9 counters.  No inline assembly, no scratch, no waits between workgroups; every buffer lives for the call only.
#include "engine.hpp"
#include "join.hpp"

#include <set>
#include <vector>

namespace llkv {

namespace {

constexpr uint32_t kMaxAggColumns = 8;
constexpr uint32_t kMaxStateLanes = 1 + 2 * kMaxAggColumns; // COUNT(*), then at most a value lane and a count lane per column
constexpr uint64_t kMaxKeySpan = 1ull << 28;
constexpr uint64_t kMaxStateBytes = 1ull << 30;
constexpr uint32_t kLookupTileRows = 8192;
constexpr uint32_t kRowsPerLane = 4;
constexpr unsigned long long kSignBit = 0x8000000000000000ull;
constexpr unsigned long long kDead = ~0ull;

enum LaneOp : uint32_t { kAddOne, kAddValid, kAddI64, kMinI64, kMaxI64, kMinF64, kMaxF64, kSumF64 /* written by the run sums */ };
enum CellFinal : uint32_t { kFinCount, kFinSumI64, kFinSumDec, kFinAvgI64, kFinSumF64, kFinTotalF64, kFinAvgF64, kFinOrderI64, kFinOrderF64 };

struct StateLane {
  const void *values;   // argument column image (8 B/row) or nullptr
  const uint8_t *valid; // its validity mask or nullptr
  uint32_t op;          // LaneOp
  uint32_t as_int;      // kSumF64: the argument is Int64, added as (double)v (TOTAL over an integer column)
};
struct StateLanes {
  StateLane lane[kMaxStateLanes];
  uint32_t n;
};
struct FinalColumn {
  uint64_t *cells;    // [span + 1]
  uint8_t *cvalid;    // [span + 1]
  uint32_t fin;       // CellFinal
  uint32_t lane_val, lane_cnt;
  uint32_t nan_default; // a NaN sum becomes the reference's default NaN (AggOut::nan_default)
};
struct FinalColumns {
  FinalColumn col[kMaxAggColumns];
  uint32_t n;
};
struct LookupColumn {
  const uint64_t *cells;
  const uint8_t *cvalid;
  unsigned long long *dst;
  uint8_t *dst_valid;
  uint32_t empty_valid; // validity of the empty-set cell (its value is zero bits for every kind)
};
struct LookupColumns {
  LookupColumn col[kMaxAggColumns];
  uint32_t n;
};

__device__ __forceinline__ long long agg_key_at(const JoinKeyColumn &k, uint64_t row) {
  if (k.width == 8) return reinterpret_cast<const long long *>(k.values)[row];
  const uint32_t v = reinterpret_cast<const uint32_t *>(k.values)[row];
  return k.is_signed ? (long long)(int32_t)v : (long long)v;
}

// order-preserving u64 images: i64 by its flipped sign bit, a finite f64 without −0.0 by the usual total-order key
__device__ __forceinline__ unsigned long long image_f64(unsigned long long bits) { return (bits & kSignBit) ? ~bits : bits | kSignBit; }
__device__ __forceinline__ unsigned long long unimage_f64(unsigned long long img) { return (img & kSignBit) ? img & ~kSignBit : ~img; }

__device__ __forceinline__ unsigned long long lane_identity(uint32_t op) { return op == kMinI64 || op == kMinF64 ? ~0ull : 0ull; }
__device__ __forceinline__ unsigned long long lane_combine(uint32_t op, unsigned long long a, unsigned long long b) {
  if (op == kMinI64 || op == kMinF64) return b < a ? b : a;
  if (op == kMaxI64 || op == kMaxF64) return b > a ? b : a;
  return a + b;
}

// rows: the qualifying inner rows (device rows, ascending).  state: [lanes.n][stride].  sort_keys (nullable): [n].
// flag bit 1: a key outside [kmin, kmin + span]
__global__ __launch_bounds__(kBlock) void agg_accumulate_kernel(JoinKeyColumn key, const uint64_t *rows, uint64_t n, long long kmin, uint64_t span, StateLanes lanes,
                                                                unsigned long long *state, uint64_t stride, uint32_t *sort_keys, uint32_t *flag) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane_id = threadIdx.x & (warpSize - 1);
  uint64_t row = 0;
  unsigned long long d = kDead;
  if (i < n) {
    row = rows[i];
    if (!key.valid || key.valid[row]) { // a NULL inner key matches nothing
      d = (unsigned long long)agg_key_at(key, row) - (unsigned long long)kmin;
      if (d > span) { atomicOr(flag, 2u); d = kDead; }
    }
    if (sort_keys) sort_keys[i] = d == kDead ? (uint32_t)span + 1u : (uint32_t)d;
  }
  // runs of equal neighbours inside the wave: head = first lane of its run, run id = heads at or before the lane
  const unsigned long long prev = __shfl_up(d, 1);
  const bool head = lane_id == 0 || prev != d;
  const unsigned long long heads = __ballot(head);
  const bool runs = heads != __ballot(1); // (uniform) some run is longer than one lane
  const uint32_t run_id = __popcll(heads & (~0ull >> (63 - lane_id)));
  const bool live = d != kDead;
  for (uint32_t l = 0; l < lanes.n; ++l) {
    const StateLane &sl = lanes.lane[l];
    if (sl.op == kSumF64) continue; // (uniform)
    unsigned long long v = lane_identity(sl.op);
    if (live) {
      const bool ok = !sl.valid || sl.valid[row];
      if (sl.op == kAddOne) v = 1;
      else if (sl.op == kAddValid) v = ok ? 1 : 0;
      else if (ok) {
        const unsigned long long bits = reinterpret_cast<const unsigned long long *>(sl.values)[row];
        v = sl.op == kAddI64 ? bits : sl.op == kMinF64 || sl.op == kMaxF64 ? image_f64(bits) : bits ^ kSignBit;
      }
    }
    if (runs) {
      for (uint32_t off = 1; off < (uint32_t)warpSize; off <<= 1) {
        const unsigned long long other = __shfl_down(v, off);
        const uint32_t other_run = __shfl_down(run_id, off);
        if (lane_id + off < (uint32_t)warpSize && other_run == run_id) v = lane_combine(sl.op, v, other);
      }
    }
    if (!live || !head || v == lane_identity(sl.op)) continue;
    unsigned long long *at = state + (uint64_t)l * stride + d;
    if (sl.op == kMinI64 || sl.op == kMinF64) atomicMin(at, v);
    else if (sl.op == kMaxI64 || sl.op == kMaxF64) atomicMax(at, v);
    else atomicAdd(at, v);
  }
}

// keys / rows: the sorted (d, device row) pairs.  The head of every run of one key adds the run left to right into every f64 lane.
__global__ __launch_bounds__(kBlock) void agg_run_sums_kernel(const uint32_t *keys, const uint64_t *rows, uint64_t n, uint64_t span, StateLanes lanes, unsigned long long *state,
                                                              uint64_t stride) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = keys[i];
  if (k > span || (i != 0 && keys[i - 1] == k)) return; // the NULL keys' run, or not the head of its run
  double acc[kMaxStateLanes];
#pragma unroll
  for (uint32_t l = 0; l < kMaxStateLanes; ++l) acc[l] = 0.0; // SumFloat64 starts at 0.0 (llkv-aggregate/src/lib.rs:870-888)
  for (uint64_t j = i; j < n && keys[j] == k; ++j) {
    const uint64_t row = rows[j];
#pragma unroll // (fully: acc stays in registers)
    for (uint32_t l = 0; l < kMaxStateLanes; ++l) {
      if (l >= lanes.n || lanes.lane[l].op != kSumF64) continue;
      const StateLane &sl = lanes.lane[l];
      if (sl.valid && !sl.valid[row]) continue;
      acc[l] += sl.as_int ? (double)reinterpret_cast<const long long *>(sl.values)[row] : reinterpret_cast<const double *>(sl.values)[row];
    }
  }
#pragma unroll
  for (uint32_t l = 0; l < kMaxStateLanes; ++l)
    if (l < lanes.n && lanes.lane[l].op == kSumF64) state[(uint64_t)l * stride + k] = (unsigned long long)__double_as_longlong(acc[l]);
}

__global__ __launch_bounds__(kBlock) void agg_finalise_kernel(const unsigned long long *state, uint64_t stride, uint64_t n_keys, FinalColumns cols) {
  for (uint64_t d = (uint64_t)blockIdx.x * kBlock + threadIdx.x; d < n_keys; d += (uint64_t)gridDim.x * kBlock) {
    for (uint32_t c = 0; c < cols.n; ++c) {
      const FinalColumn &fc = cols.col[c];
      const unsigned long long cnt = state[(uint64_t)fc.lane_cnt * stride + d];
      unsigned long long v = state[(uint64_t)fc.lane_val * stride + d];
      if (fc.nan_default) {
        const double s = __longlong_as_double((long long)v);
        if (s != s) v = 0xFFF8000000000000ull;
      }
      bool ok = cnt != 0;
      switch (fc.fin) {
      case kFinCount: v = cnt; ok = true; break;
      case kFinSumDec: ok = true; break; // `vec![sum]`: 0, never NULL, even without rows
      case kFinTotalF64: ok = true; break;
      case kFinAvgI64: if (ok) v = (unsigned long long)__double_as_longlong((double)(long long)v / (double)(long long)cnt); break;
      case kFinAvgF64: if (ok) v = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)v) / (double)(long long)cnt); break;
      case kFinOrderI64: v ^= kSignBit; break;
      case kFinOrderF64: v = unimage_f64(v); break;
      default: break; // kFinSumI64, kFinSumF64: the lane itself
      }
      fc.cells[d] = ok ? v : 0ull; // NULL cells hold zero values
      fc.cvalid[d] = ok ? 1 : 0;
    }
  }
}

// counters[0] = outer rows whose key has a qualifying inner row, counters[1 + c] = present cells of column c
__global__ __launch_bounds__(kBlock) void agg_lookup_kernel(JoinKeyColumn key, const TileDesc *tiles, uint32_t n_tiles, const unsigned long long *count_star, long long kmin,
                                                            uint64_t span, LookupColumns cols, unsigned long long *counters) {
  __shared__ uint32_t block_count[1 + kMaxAggColumns];
  if (threadIdx.x <= kMaxAggColumns) block_count[threadIdx.x] = 0;
  __syncthreads();
  uint32_t my_count[1 + kMaxAggColumns];
#pragma unroll
  for (uint32_t c = 0; c <= kMaxAggColumns; ++c) my_count[c] = 0;

  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const TileDesc tile = tiles[t];
    for (uint32_t r = threadIdx.x * kRowsPerLane; r < tile.rows; r += kBlock * kRowsPerLane) {
      const uint64_t at = tile.dev_row + r; // a multiple of 4: tiles start on 16-row boundaries of the image
      const uint32_t live = tile.rows - r < kRowsPerLane ? tile.rows - r : kRowsPerLane;
      long long k[kRowsPerLane];
      if (key.width == 8) {
        const longlong2 a = reinterpret_cast<const longlong2 *>(key.values)[at / 2], b = reinterpret_cast<const longlong2 *>(key.values)[at / 2 + 1];
        k[0] = a.x; k[1] = a.y; k[2] = b.x; k[3] = b.y;
      } else {
        const uint4 a = reinterpret_cast<const uint4 *>(key.values)[at / 4];
        const uint32_t w[kRowsPerLane] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (uint32_t j = 0; j < kRowsPerLane; ++j) k[j] = key.is_signed ? (long long)(int32_t)w[j] : (long long)w[j];
      }
      const uint32_t kvalid = key.valid ? reinterpret_cast<const uint32_t *>(key.valid)[at / 4] : 0x01010101u;
      unsigned long long d[kRowsPerLane]; // kDead: a NULL key, a key outside the inner range, a padding row
      bool in_range[kRowsPerLane];
#pragma unroll
      for (uint32_t j = 0; j < kRowsPerLane; ++j) {
        d[j] = (unsigned long long)k[j] - (unsigned long long)kmin; // (wraps: INT64_MIN under a positive min is out of range)
        in_range[j] = j < live && ((kvalid >> (8 * j)) & 0xffu) != 0 && d[j] <= span;
        my_count[0] += in_range[j] && count_star[d[j]] != 0;
      }
#pragma unroll // (fully: my_count stays in registers)
      for (uint32_t c = 0; c < kMaxAggColumns; ++c) {
        if (c >= cols.n) continue;
        const LookupColumn &lc = cols.col[c];
        uint32_t present = 0; // byte j = 1: cell j is not NULL
        unsigned long long v[kRowsPerLane];
#pragma unroll
        for (uint32_t j = 0; j < kRowsPerLane; ++j) {
          const bool ok = in_range[j] ? lc.cvalid[d[j]] != 0 : (j < live && lc.empty_valid);
          v[j] = in_range[j] && ok ? lc.cells[d[j]] : 0ull; // the empty-set cell's value is zero bits
          if (ok) present |= 1u << (8 * j);
        }
        reinterpret_cast<ulonglong2 *>(lc.dst)[at / 2] = make_ulonglong2(v[0], v[1]);
        reinterpret_cast<ulonglong2 *>(lc.dst)[at / 2 + 1] = make_ulonglong2(v[2], v[3]);
        reinterpret_cast<uint32_t *>(lc.dst_valid)[at / 4] = present;
        my_count[1 + c] += __popc(present);
      }
    }
  }

  // per wave, then per workgroup, then one atomic per counter
#pragma unroll
  for (uint32_t c = 0; c <= kMaxAggColumns; ++c) {
    if (c > cols.n) continue; // (uniform)
    uint32_t v = my_count[c];
    for (int off = warpSize / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & (warpSize - 1)) == 0 && v) atomicAdd(&block_count[c], v);
  }
  __syncthreads();
  if (threadIdx.x <= cols.n && block_count[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)block_count[threadIdx.x]);
}

int aggregate_key_of(const Table *t, uint32_t field, const char *side, const DeviceColumn **out) {
  auto it = t->cols.find(field);
  if (it == t->cols.end()) return set_error(LLKV_NOT_FOUND, std::string("aggregate columns: ") + side + " key field " + std::to_string(field) + " is not staged");
  switch (it->second.info.dtype) {
  case LLKV_DT_INT64: case LLKV_DT_INT32: case LLKV_DT_DATE32: case LLKV_DT_UINT32: break;
  default: return set_error(LLKV_UNSUPPORTED, std::string("aggregate columns: the ") + side + " key must be Int64, Int32, Date32 or UInt32, got " + dtype_name(it->second.info.dtype));
  }
  *out = &it->second;
  return LLKV_OK;
}

const char *kind_name(int32_t kind) {
  switch (kind) {
  case LLKV_AGG_COUNT_STAR: return "COUNT(*)";
  case LLKV_AGG_COUNT: return "COUNT";
  case LLKV_AGG_SUM: return "SUM";
  case LLKV_AGG_TOTAL: return "TOTAL";
  case LLKV_AGG_AVG: return "AVG";
  case LLKV_AGG_MIN: return "MIN";
  case LLKV_AGG_MAX: return "MAX";
  default: return "?";
  }
}

// What one requested column becomes: its output type, its lanes in the per-key state, its finalisation.
struct ColumnPlan {
  const DeviceColumn *arg = nullptr; // nullptr: COUNT(*)
  int32_t dtype = LLKV_DT_INT64, precision = 0, scale = 0;
  uint32_t fin = kFinCount, lane_val = 0, lane_cnt = 0;
  bool nan_default = false, empty_valid = true;
};

struct LanePlanner {
  StateLanes lanes{};
  LanePlanner() { lanes.n = 1; lanes.lane[0] = StateLane{nullptr, nullptr, kAddOne, 0}; } // lane 0: COUNT(*) of every key
  uint32_t add(const DeviceColumn &c, uint32_t op, uint32_t as_int = 0) {
    const void *values = op == kAddValid ? nullptr : c.d_values.get();
    const uint8_t *valid = c.info.nullable ? c.d_valid.get<uint8_t>() : nullptr;
    for (uint32_t l = 0; l < lanes.n; ++l)
      if (lanes.lane[l].op == op && lanes.lane[l].values == values && lanes.lane[l].valid == valid && lanes.lane[l].as_int == as_int && op != kAddOne) return l;
    lanes.lane[lanes.n] = StateLane{values, valid, op, as_int};
    return lanes.n++;
  }
  // rows of the key whose argument cell is not NULL: COUNT(*)'s lane when the column has no NULL cell
  uint32_t count_of(const DeviceColumn &c) { return c.info.nullable ? add(c, kAddValid) : 0; }
};

// The ungrouped aggregate's own rules (plan.cpp: AggLowering::one / numeric / decimal64, engine.cpp: finalize_value) for a bare column.
int plan_column(const Table *ti, const llkv_table_aggregate_column &spec, LanePlanner *lp, ColumnPlan *out) {
  const std::string where = std::string("aggregate columns: ") + kind_name(spec.kind);
  if (spec.kind == LLKV_AGG_COUNT_STAR) return LLKV_OK; // (the defaults: lane 0, Int64, never NULL; the caller admitted the kind)
  auto it = ti->cols.find(spec.inner_field);
  if (it == ti->cols.end()) return set_error(LLKV_NOT_FOUND, "aggregate columns: inner field " + std::to_string(spec.inner_field) + " is not staged");
  const DeviceColumn &c = it->second;
  const ColumnInfo &ci = c.info;
  const std::string arg = where + " over inner field " + std::to_string(spec.inner_field);
  out->arg = &c;
  out->lane_cnt = lp->count_of(c);
  if (spec.kind == LLKV_AGG_COUNT) { out->lane_val = out->lane_cnt; return LLKV_OK; } // any staged column: only its validity is read
  if (ci.wide128) return set_error(LLKV_UNSUPPORTED, arg + ": a Decimal128 column with values beyond 64 bits (a wide decimal)");
  if (ci.dtype != LLKV_DT_INT64 && ci.dtype != LLKV_DT_FLOAT64 && ci.dtype != LLKV_DT_DECIMAL128)
    return set_error(LLKV_UNSUPPORTED, arg + ": the argument must be an Int64, Float64 or Decimal128 column, got " + dtype_name(ci.dtype));
  const bool is_dec = ci.dtype == LLKV_DT_DECIMAL128, is_f64 = ci.dtype == LLKV_DT_FLOAT64;
  if (is_dec && spec.kind == LLKV_AGG_AVG) return set_error(LLKV_UNSUPPORTED, arg + ": AVG over Decimal128 is not an aggregate column (COUNT / SUM / MIN / MAX are)");
  if (is_dec && spec.kind == LLKV_AGG_TOTAL) return set_error(LLKV_UNSUPPORTED, arg + ": TOTAL over Decimal128 is not an aggregate column (COUNT / SUM / MIN / MAX are)");
  out->empty_valid = false;
  if (spec.kind == LLKV_AGG_MIN || spec.kind == LLKV_AGG_MAX) {
    const bool is_min = spec.kind == LLKV_AGG_MIN;
    out->dtype = ci.dtype; out->precision = ci.precision; out->scale = ci.scale;
    if (is_f64) {
      // MinFloat64 / MaxFloat64 fold by partial_cmp in row order (a leading NaN sticks, ±0 ties keep the earlier row): order-free
      // exactly when the statistics exclude both, the rule of the ungrouped aggregate's one-lane form (plan.cpp: plain_f64)
      if (ci.rows != 0 && (!ci.has_fstats || !ci.f_all_finite || !ci.f_no_neg_zero)) // (an empty table has no cell and no statistics)
        return set_error(LLKV_UNSUPPORTED, arg + ": MIN / MAX over a Float64 column need all_finite statistics without −0.0 (the reference's fold is order dependent otherwise)");
      out->fin = kFinOrderF64;
      out->lane_val = lp->add(c, is_min ? kMinF64 : kMaxF64);
    } else {
      out->fin = kFinOrderI64;
      out->lane_val = lp->add(c, is_min ? kMinI64 : kMaxI64);
    }
    return LLKV_OK;
  }
  if (is_f64 || spec.kind == LLKV_AGG_TOTAL) { // f64 accumulation in row order: TOTAL over Int64 adds (double)v
    out->dtype = LLKV_DT_FLOAT64;
    out->fin = spec.kind == LLKV_AGG_SUM ? kFinSumF64 : spec.kind == LLKV_AGG_AVG ? kFinAvgF64 : kFinTotalF64;
    out->empty_valid = spec.kind == LLKV_AGG_TOTAL;
    out->nan_default = is_f64 && ci.f_no_nan;
    out->lane_val = lp->add(c, kSumF64, is_f64 ? 0 : 1);
    return LLKV_OK;
  }
  // integer and decimal sums: one wrapping lane, admitted when the statistics exclude i64 overflow of any prefix (plan.cpp: fast_i64)
  const unsigned __int128 lo = (unsigned __int128)(ci.min_i < 0 ? -(__int128)ci.min_i : (__int128)ci.min_i), hi = (unsigned __int128)(ci.max_i < 0 ? -(__int128)ci.max_i : (__int128)ci.max_i);
  const unsigned __int128 mag = lo > hi ? lo : hi;
  if (ci.rows != 0 && (!ci.has_stats || mag * (unsigned __int128)ci.rows > (unsigned __int128)INT64_MAX)) // (an empty table has no statistics)
    return set_error(LLKV_UNSUPPORTED, arg + ": possible i64 overflow (rows · max|v| may exceed i64" + (ci.has_stats ? "" : ": the column has no statistics") +
                                           "): the reference's check is order dependent");
  out->lane_val = lp->add(c, kAddI64);
  if (spec.kind == LLKV_AGG_AVG) { out->dtype = LLKV_DT_FLOAT64; out->fin = kFinAvgI64; return LLKV_OK; }
  if (is_dec) { // SumDecimal128 keeps the column's (precision, scale) and is 0, never NULL, over no rows
    out->dtype = LLKV_DT_DECIMAL128; out->precision = ci.precision; out->scale = ci.scale;
    out->fin = kFinSumDec;
    out->empty_valid = true;
    return LLKV_OK;
  }
  out->dtype = LLKV_DT_INT64;
  out->fin = kFinSumI64;
  return LLKV_OK;
}

} // namespace

static int add_aggregate_columns(Table *to, uint32_t outer_key_field, const llkv_join_side *inner, const llkv_table_aggregate_column *cols, uint32_t n_cols,
                                 uint64_t *matched_rows) {
  // ---- what needs no device -------------------------------------------------------------------------------------------------------
  if (!to || !inner || !inner->table || !cols || (inner->n_filters && !inner->filters)) return set_error(LLKV_INVALID_ARGUMENT, "aggregate columns: NULL argument");
  if (n_cols == 0 || n_cols > kMaxAggColumns)
    return set_error(LLKV_INVALID_ARGUMENT, "aggregate columns: n_cols must be 1.." + std::to_string(kMaxAggColumns) + ", got " + std::to_string(n_cols));
  std::set<uint32_t> outs;
  for (uint32_t c = 0; c < n_cols; ++c)
    if (!outs.insert(cols[c].out_field).second) return set_error(LLKV_INVALID_ARGUMENT, "aggregate columns: out_field " + std::to_string(cols[c].out_field) + " is listed twice");
  for (uint32_t c = 0; c < n_cols; ++c) {
    if (cols[c].kind == LLKV_AGG_COUNT_NULLS) return set_error(LLKV_UNSUPPORTED, "aggregate columns: COUNT_NULLS is not an aggregate column kind");
    if (cols[c].kind < LLKV_AGG_COUNT_STAR || cols[c].kind > LLKV_AGG_COUNT_NULLS) return set_error(LLKV_INVALID_ARGUMENT, "aggregate columns: aggregate kind " + std::to_string(cols[c].kind));
  }
  const Table *ti = reinterpret_cast<const Table *>(inner->table);
  if (to->world != 1 || ti->world != 1) return set_error(LLKV_UNSUPPORTED, "aggregate columns: sharded tables (world != 1) are not supported");
  int rc;
  for (uint32_t c = 0; c < n_cols; ++c)
    if ((rc = check_new_column(to, cols[c].out_field, to->n_local_chunks))) return rc;
  const DeviceColumn *ko = nullptr, *ki = nullptr;
  if ((rc = aggregate_key_of(to, outer_key_field, "outer", &ko)) || (rc = aggregate_key_of(ti, inner->key_field, "inner", &ki))) return rc;
  LanePlanner lp;
  ColumnPlan plan[kMaxAggColumns];
  bool f64_sums = false;
  for (uint32_t c = 0; c < n_cols; ++c) {
    if ((rc = plan_column(ti, cols[c], &lp, &plan[c]))) return rc;
    f64_sums |= plan[c].fin == kFinSumF64 || plan[c].fin == kFinAvgF64 || plan[c].fin == kFinTotalF64;
  }
  long long kmin = 0;
  uint64_t span = 0;
  if (ti->local_rows) {
    const ColumnInfo &info = ki->info;
    if (!info.has_stats || info.max_i < info.min_i) return set_error(LLKV_UNSUPPORTED, "aggregate columns: the inner key has no statistics-bounded range for a direct per-key state");
    kmin = info.min_i;
    span = (uint64_t)info.max_i - (uint64_t)info.min_i;
    if (span >= kMaxKeySpan) return set_error(LLKV_UNSUPPORTED, "aggregate columns: the inner key's range spans 2^28 keys or more");
  }
  const uint64_t stride = (span + 2) / 2 * 2; // keys per lane, a whole number of 16-byte fills
  const uint32_t n_lanes = lp.lanes.n;
  if ((span + 1) * 8 * (uint64_t)(n_lanes + n_cols) > kMaxStateBytes)
    return set_error(LLKV_UNSUPPORTED, "aggregate columns: the per-key state of " + std::to_string(n_lanes + n_cols) + " lanes over " + std::to_string(span + 1) +
                                           " keys would pass 1 GiB");
  if (ti->dev_rows >= 0xFFFFFFFFull) return set_error(LLKV_UNSUPPORTED, "aggregate columns: an inner image of 2^32 rows or more");
  if ((rc = ensure_device())) return rc;
  hipStream_t s = g_ctx.stream;
  PhaseTrace trace("[llkv aggregate_column] %-22s %9.3f ms\n", s);

  // ---- selection: the qualifying inner rows, ascending ----------------------------------------------------------------------------
  Selection sel;
  if (ti->local_rows && (rc = run_selection(ti, inner->filters, inner->n_filters, nullptr, 0, &sel))) return rc;
  trace.mark("selection");

  // ---- accumulate: the order-free lanes, and the sort keys of the f64 sums --------------------------------------------------------
  DeviceBuffer d_state, d_words, d_keys_in;
  HIP_TRY(d_state.alloc((uint64_t)n_lanes * stride, 8));
  HIP_TRY(d_words.alloc(2 + kMaxAggColumns, 8)); // [0]: the accumulate pass's flag word, [1 …]: the lookup's counters
  HIP_TRY(hipMemsetAsync(d_words.get(), 0, (2 + kMaxAggColumns) * 8, s));
  for (uint32_t l = 0; l < n_lanes; ++l) {
    const uint32_t op = lp.lanes.lane[l].op;
    HIP_TRY(hj_launch_fill(d_state.get<uint64_t>() + (uint64_t)l * stride, stride * 8, op == kMinI64 || op == kMinF64 ? ~0ull : 0ull, s));
  }
  const bool sorting = f64_sums && sel.n != 0;
  if (sorting) HIP_TRY(d_keys_in.alloc(sel.n, 4));
  uint32_t flag = 0;
  if (sel.n) {
    hipLaunchKernelGGL(agg_accumulate_kernel, dim3((uint32_t)((sel.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, key_view(*ki), sel.d_dev, sel.n, kmin, span, lp.lanes,
                       d_state.get<unsigned long long>(), stride, sorting ? d_keys_in.get<uint32_t>() : nullptr, d_words.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&flag, d_words.get(), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  trace.mark("accumulate");
  if (flag & 2u) return set_error(LLKV_INTERNAL, "aggregate columns: an inner key lies outside the column's statistics");

  // ---- f64 sums: stable sort by key, then every run added left to right -----------------------------------------------------------
  if (sorting) {
    uint32_t bits = 1;
    while (bits < 32 && ((span + 1) >> bits) != 0) ++bits; // the NULL keys' bucket span + 1 included
    DeviceBuffer d_keys_out, d_rows_out, d_tmp;
    HIP_TRY(d_keys_out.alloc(sel.n, 4));
    HIP_TRY(d_rows_out.alloc(sel.n, 8));
    size_t tmp_bytes = 0;
    HIP_TRY(hj_sort_u32_u64(nullptr, &tmp_bytes, d_keys_in.get<uint32_t>(), d_keys_out.get<uint32_t>(), sel.d_dev, d_rows_out.get<uint64_t>(), sel.n, bits, s));
    HIP_TRY(d_tmp.alloc(tmp_bytes ? tmp_bytes : 16, 1));
    HIP_TRY(hj_sort_u32_u64(d_tmp.get(), &tmp_bytes, d_keys_in.get<uint32_t>(), d_keys_out.get<uint32_t>(), sel.d_dev, d_rows_out.get<uint64_t>(), sel.n, bits, s));
    trace.mark("sort");
    hipLaunchKernelGGL(agg_run_sums_kernel, dim3((uint32_t)((sel.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_keys_out.get<uint32_t>(), d_rows_out.get<uint64_t>(), sel.n, span,
                       lp.lanes, d_state.get<unsigned long long>(), stride);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s)); // (the sort buffers are freed on leaving the block)
    trace.mark("run sums");
  }

  // ---- finalise: one cell image and one validity byte per key and column ----------------------------------------------------------
  DeviceBuffer d_cells, d_cvalid;
  const uint64_t vstride = (span + 16) / 16 * 16;
  HIP_TRY(d_cells.alloc((uint64_t)n_cols * stride, 8));
  HIP_TRY(d_cvalid.alloc((uint64_t)n_cols * vstride, 1));
  FinalColumns fin{};
  fin.n = n_cols;
  for (uint32_t c = 0; c < n_cols; ++c)
    fin.col[c] = FinalColumn{d_cells.get<uint64_t>() + (uint64_t)c * stride, d_cvalid.get<uint8_t>() + (uint64_t)c * vstride, plan[c].fin, plan[c].lane_val, plan[c].lane_cnt,
                             plan[c].nan_default ? 1u : 0u};
  {
    const uint64_t blocks = (span + kBlock) / kBlock;
    const uint32_t grid = (uint32_t)(blocks < (uint64_t)g_ctx.cu_count * 8 ? blocks : (uint64_t)g_ctx.cu_count * 8);
    hipLaunchKernelGGL(agg_finalise_kernel, dim3(grid), dim3(kBlock), 0, s, d_state.get<unsigned long long>(), stride, span + 1, fin);
    HIP_TRY(hipGetLastError());
  }
  trace.mark("finalise");

  // ---- lookup: one pass over the outer image fills every column --------------------------------------------------------------------
  std::vector<DeviceColumn> made(n_cols);
  LookupColumns look{};
  look.n = n_cols;
  for (uint32_t c = 0; c < n_cols; ++c) {
    DeviceColumn &m = made[c];
    m.info.field_id = cols[c].out_field;
    m.info.dtype = plan[c].dtype;
    m.info.rows = to->total_rows;
    m.info.precision = plan[c].precision;
    m.info.scale = plan[c].scale;
    m.join_column = true; // every lifetime rule of a join column: a snapshot, dropped with them, appends refuse while it is there
    m.src_table_id = ti->table_id;
    m.src_generation = ti->generation;
    m.src_field = plan[c].arg ? cols[c].inner_field : inner->key_field;
    if ((rc = alloc_column(*to, 8, m.d_values)) || (rc = alloc_column(*to, 1, m.d_valid))) return rc;
    look.col[c] = LookupColumn{fin.col[c].cells, fin.col[c].cvalid, m.d_values.get<unsigned long long>(), m.d_valid.get<uint8_t>(), plan[c].empty_valid ? 1u : 0u};
  }
  const TileSet *ts = nullptr;
  if ((rc = get_tileset(*to, kLookupTileRows, &ts))) return rc;
  if (ts->n_tiles) {
    const uint32_t grid = ts->n_tiles < g_ctx.cu_count * 8 ? ts->n_tiles : g_ctx.cu_count * 8;
    hipLaunchKernelGGL(agg_lookup_kernel, dim3(grid), dim3(kBlock), 0, s, key_view(*ko), ts->d_tiles.get<TileDesc>(), ts->n_tiles, d_state.get<unsigned long long>(), kmin, span,
                       look, d_words.get<unsigned long long>() + 1);
    HIP_TRY(hipGetLastError());
  }
  unsigned long long counts[1 + kMaxAggColumns] = {0};
  HIP_TRY(hipMemcpyAsync(counts, d_words.get<unsigned long long>() + 1, sizeof counts, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  trace.mark("lookup");

  // ---- registration: as a column staged from the host — a mask only when some cell is NULL, statistics over the result -------------
  for (uint32_t c = 0; c < n_cols; ++c) {
    DeviceColumn &m = made[c];
    m.info.nullable = counts[1 + c] != to->local_rows;
    if (!m.info.nullable) m.d_valid.reset();
  }
  std::map<uint32_t, DeviceColumn> staged;
  for (uint32_t c = 0; c < n_cols; ++c)
    if ((rc = register_column(*to, staged, cols[c].out_field, std::move(made[c])))) return rc;
  for (auto &kv : staged) to->cols.emplace(kv.first, std::move(kv.second));
  trace.mark("statistics");
  if (matched_rows) *matched_rows = counts[0];
  return LLKV_OK;
}

} // namespace llkv

extern "C" {

llkv_status llkv_hip_table_add_aggregate_columns(llkv_hip_table *outer, uint32_t outer_key_field, const llkv_join_side *inner, const llkv_table_aggregate_column *cols,
                                                 uint32_t n_cols, uint64_t *matched_rows) {
  return (llkv_status)llkv::add_aggregate_columns(reinterpret_cast<llkv::Table *>(outer), outer_key_field, inner, cols, n_cols, matched_rows);
}

} // extern "C"
