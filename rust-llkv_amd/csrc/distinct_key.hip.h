// distinct_key.hip.h — what the calls that deduplicate the rows of a projection scan in HBM share: llkv_hip_scan_distinct
// (scan_distinct.hip) and llkv_hip_scan_setop (scan_setop.hip).  The column descriptor and the 64-bit word of a staged cell, the
// row hash, the two inserts that leave the smallest selection index of every class of equal rows in a table of uint32 cells, and
// the compaction of the flagged rows into a new Selection.  The argument why the tables end the same whatever the timing is
// written out at the head of scan_distinct.hip.
#pragma once
#include "engine.hpp"

#include <algorithm>

namespace llkv {

// kDistF64: SELECT DISTINCT's CanonicalRow (every NaN one class, −0.0 as +0.0); kDistF64Bits: the compound SELECT's encode_row (the bits)
enum DistinctKind : int32_t { kDistSigned = 0, kDistBool = 1, kDistF64 = 2, kDistCode = 3, kDistF64Bits = 4 };
enum DistinctError : uint32_t { kDistErrProbes = 1, kDistErrRange = 2, kDistErrIndex = 4 };
constexpr uint32_t kDistEmpty = 0xFFFFFFFFu;
constexpr uint32_t kDistBlock = 256;
constexpr uint64_t kDirectMaxCells = 1ull << 24; // the direct route's table: at most 64 MiB of cells

struct DistinctCol {
  const void *values;
  const uint8_t *valid;    // 1 B/row validity mask, nullptr: the column has no NULL cell
  const uint32_t *map;     // kDistCode: code → the word that stands for its string (nullptr: the code itself)
  unsigned long long map_n; // … its entries
  long long base;          // direct route: the smallest value the statistics admit (codes, Boolean: 0)
  unsigned long long card; // direct route: how many values they admit
  unsigned long long stride; // direct route: the weight of this column's digit
  int32_t width, kind;
  int32_t null_digit, pad; // direct route: 1 = digit 0 stands for NULL, a valid cell's digit is one up
};

struct DistinctParams {
  const uint64_t *dev; // selection index → device row
  uint64_t n;
  int32_t n_cols, pad;
  DistinctCol c[kMaxOuts];
};

__device__ inline bool dist_null(const DistinctCol &c, uint64_t dev) { return c.valid && !c.valid[dev]; }

// the word of a valid cell: equal cells, equal words
__device__ inline uint64_t dist_word(const DistinctCol &c, uint64_t dev) {
  const uint64_t raw = c.width == 8 ? static_cast<const uint64_t *>(c.values)[dev]
                     : c.width == 4 ? (uint64_t) static_cast<const uint32_t *>(c.values)[dev]
                                    : (uint64_t) static_cast<const uint8_t *>(c.values)[dev];
  switch (c.kind) {
  case kDistSigned: return c.width == 8 ? raw : (uint64_t)(int64_t)(int32_t)raw;
  case kDistBool: return raw != 0 ? 1u : 0u;
  case kDistF64:
    if ((raw & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return 0x7FF8000000000000ull; // FloatNaN: one class
    return (raw << 1) == 0 ? 0ull : raw;                                                      // −0.0 and +0.0: one class
  case kDistCode:
    if (!c.map) return raw;
    return raw < c.map_n ? (uint64_t)c.map[raw] : ~0ull; // (a code outside its dictionary: never an address)
  default: return raw; // kDistF64Bits
  }
}

__device__ inline uint64_t dist_mix(uint64_t h, uint64_t w) {
  h = (h ^ w) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}

__device__ inline uint64_t dist_hash(const DistinctParams &p, uint64_t dev) {
  uint64_t h = 0x243F6A8885A308D3ull;
  for (int j = 0; j < p.n_cols; ++j) h = dist_null(p.c[j], dev) ? dist_mix(h, 0xC2B2AE3D27D4EB4Full + (uint64_t)j) : dist_mix(h, dist_word(p.c[j], dev));
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  return h ^ (h >> 33);
}

// equality of the row at device row a of p and the row at device row b of q (the same columns, maybe of two tables): every column
// NULL in both, or valid in both with the same word
__device__ inline bool dist_equal(const DistinctParams &p, uint64_t a, const DistinctParams &q, uint64_t b) {
  for (int j = 0; j < p.n_cols; ++j) {
    const bool na = dist_null(p.c[j], a), nb = dist_null(q.c[j], b);
    if (na != nb) return false;
    if (!na && dist_word(p.c[j], a) != dist_word(q.c[j], b)) return false;
  }
  return true;
}

// the direct route's cell of a row: its mixed-radix key; false = a valid cell lies outside its column's statistics
__device__ inline bool dist_direct_key(const DistinctParams &p, uint64_t dev, uint64_t *key) {
  bool inside = true;
  uint64_t k = 0;
  for (int j = 0; j < p.n_cols; ++j) {
    const DistinctCol &c = p.c[j];
    uint64_t digit = 0; // NULL
    if (!dist_null(c, dev)) {
      const uint64_t d = dist_word(c, dev) - (uint64_t)c.base;
      inside &= d < c.card;
      digit = d + (uint64_t)c.null_digit;
    }
    k += digit * c.stride;
  }
  *key = k;
  return inside;
}

namespace {

__global__ __launch_bounds__(kDistBlock) void distinct_direct_insert(DistinctParams p, uint32_t *cells, uint64_t n_cells, uint32_t *error) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t rounds = (p.n + stride - 1) / stride; // every lane of a wave makes every round: the wave looks at its keys together
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t r = 0; r < rounds; ++r) {
    const uint64_t i = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool live = i < p.n;
    uint64_t key = 0;
    if (live && (!dist_direct_key(p, p.dev[i], &key) || key >= n_cells)) { // (a cell the statistics do not cover: never an address)
      atomicOr(error, (uint32_t)kDistErrRange);
      live = false;
    }
    // Few classes are the case this route is for: the lanes of a wave that share a cell leave it to the lowest of them, which has
    // the smallest index (64 loads of one address become one); four cells are looked for, whoever is left goes on for itself.
    uint64_t todo = __ballot(live);
    for (int k = 0; k < 4 && todo; ++k) {
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const uint64_t theirs = ((uint64_t)(uint32_t)__shfl((int)(key >> 32), leader) << 32) | (uint32_t)__shfl((int)key, leader);
      const uint64_t same = __ballot(live && key == theirs);
      if (live && key == theirs && lane != (uint32_t)leader) live = false;
      todo &= ~same;
    }
    if (live && (uint32_t)i < __hip_atomic_load(cells + key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      __hip_atomic_fetch_min(cells + key, (uint32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(kDistBlock) void distinct_hash_insert(DistinctParams p, uint32_t *slots, uint64_t cap_mask, uint64_t hash_mask, uint32_t *error) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += stride) {
    const uint64_t dev = p.dev[i];
    uint64_t at = dist_hash(p, dev) & hash_mask & cap_mask;
    for (uint64_t probes = 0;; ++probes, at = (at + 1) & cap_mask) {
      if (probes > cap_mask) { // every slot seen: the table is broken (it holds at most n <= capacity / 2 classes)
        atomicOr(error, (uint32_t)kDistErrProbes);
        break;
      }
      uint32_t v = __hip_atomic_load(slots + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v == kDistEmpty) {
        uint32_t seen = kDistEmpty;
        if (__hip_atomic_compare_exchange_strong(slots + at, &seen, (uint32_t)i, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break; // claimed
        v = seen; // somebody's row arrived first: is it one of mine?
      }
      if (v >= p.n) { // (not an index of the selection: never an address)
        atomicOr(error, (uint32_t)kDistErrIndex);
        break;
      }
      if (dist_equal(p, dev, p, p.dev[v])) {
        if (v > (uint32_t)i) __hip_atomic_fetch_min(slots + at, (uint32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
  }
}

__global__ __launch_bounds__(kDistBlock) void distinct_compact(const uint64_t *flags, const uint64_t *offsets, uint64_t n, uint64_t n_out, const uint64_t *dev, const uint64_t *ids,
                                                               uint64_t *out_dev, uint64_t *out_ids) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flags[i]) return;
  const uint64_t at = offsets[i];
  if (at >= n_out) return;
  out_dev[at] = dev[i];
  out_ids[at] = ids[i];
}

} // namespace

inline uint32_t dist_grid(uint64_t n) {
  const uint64_t want = (n + kDistBlock - 1) / kDistBlock, cap = (uint64_t)g_ctx.cu_count * 16;
  return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}

// The column's descriptor; *card = how many values the statistics admit (0: they bound nothing — the hash route).  `float_bits`:
// a Float64 cell stands for its bits (kDistF64Bits) instead of its canonical form.
inline void describe_column(const DeviceColumn &c, DistinctCol *d, unsigned __int128 *card, bool float_bits = false) {
  const ColumnInfo &ci = c.info;
  d->values = c.d_values.get();
  d->valid = ci.nullable ? c.d_valid.get<uint8_t>() : nullptr;
  d->map = nullptr;
  d->map_n = 0;
  d->base = 0;
  d->card = d->stride = 0;
  d->width = (int32_t)dtype_width(storage_dtype(ci));
  d->null_digit = d->valid ? 1 : 0;
  d->pad = 0;
  *card = 0;
  switch (ci.dtype) {
  case LLKV_DT_FLOAT64: d->kind = float_bits ? kDistF64Bits : kDistF64; break;
  case LLKV_DT_BOOLEAN: d->kind = kDistBool; *card = 2; break;
  case LLKV_DT_UTF8: d->kind = kDistCode; *card = std::max<size_t>(1, ci.dictionary.size()); break;
  case LLKV_DT_DECIMAL128: d->kind = kDistSigned; break; // (narrowed to 64 bits; its raw range is left to the hash route)
  default: // Int64, Date32
    d->kind = kDistSigned;
    if (ci.has_stats && ci.max_i >= ci.min_i) {
      d->base = ci.min_i;
      *card = (unsigned __int128)((__int128)ci.max_i - (__int128)ci.min_i) + 1;
    }
  }
}

} // namespace llkv
