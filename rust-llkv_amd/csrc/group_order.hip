// group_order.hip — ORDER BY output columns, then OFFSET / LIMIT, over the groups of a GROUP BY
// (sort_record_batch_with_order llkv-executor/src/lib.rs:13762-13868, SelectExecution::stream :10918-10955).
//
// Device top-k (sort-based and partitioned routes, offset + limit ≤ kGroupOrderDeviceRows), over the groups the route left in
// HBM in their unordered output order ([n][k] lanes, [n_keys][n] key cells and validity):
//   order keys   order_key_kernel    per group and term: a NULL word (0 / 1 by NULLS FIRST / LAST) and one or two value words,
//                                    an order-preserving unsigned image of the cell the host finalize returns (i64: sign bit
//                                    flipped, f64: the total_cmp flip, Decimal128: two words, Utf8: rank of the dictionary
//                                    code; DESC: complemented).  The same pass records, per aggregate whose finalize can fail
//                                    (i64 SUM / AVG), the first group that fails — the host then finalizes that one group for
//                                    the status and message of the unordered query.
//   select       order_radix_pass    exact radix select of the first m = offset + limit groups over the composite key (the
//                                    words, then the position = the tie break): one 8-bit digit per launch, a histogram of the
//                                    groups still tied with the threshold; the last workgroup to arrive picks the digit and
//                                    moves the threshold (no workgroup waits for another).  Words whose upper bytes are known
//                                    to be zero (NULL words, positions) skip those digits; once the tied groups are exactly
//                                    the ones still needed the remaining launches return at once.
//                order_select_kernel the m groups at or below the threshold
//   rank         order_rank_kernel   each survivor counts the survivors below it (LDS tiles of 128): its output position
//   gather       order_gather_kernel rows [offset, m) in order → copied out (only those)
// Host order (group_order_host): the same images from the finalized cells, std::partial_sort — the dense routes, the merged
// groups of a sharded table, larger limits and terms without a device form (a computed DECIMAL argument's precision check).
#include "engine.hpp"
#include "group_cell.hip.h"
#include "order_select.hip.h"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

namespace llkv {

namespace {

enum TermKind : int32_t { kTermKeyInt = 0, kTermKeyUtf8 = 1, kTermAgg = 2 };

struct OrderTerm {
  int32_t kind, key;        // key terms: the key's index
  int32_t word;             // first key word of the term
  int32_t desc, nulls_first;
  AggCell a;                // aggregate terms: what the device finalize needs
  const uint32_t *rank; // Utf8 keys: dictionary code → position in byte order
};

struct OrderParams {
  const uint64_t *lanes;
  const int64_t *kv;
  const uint8_t *kvalid;
  uint64_t n;
  int32_t k, n_terms, n_words, n_err;
  uint64_t *keys;                // [n_words][n]
  unsigned long long *first_bad; // [n_err]: smallest group whose finalize of that aggregate fails
  int32_t err_lane[kMaxErrAggs], err_count_lane[kMaxErrAggs];
  OrderTerm t[kMaxTerms];
};

// order-preserving unsigned image of a finalized cell (group_cell.hip.h: agg_cell): *null, or the value's words (one, two for Decimal128)
__device__ inline void agg_image(const AggCell &a, const uint64_t *g, bool *null, uint64_t *w0, uint64_t *w1) {
  agg_cell(a, g, null, w0, w1);
  if (*null) return;
  switch (agg_cell_type((AggFinal)a.fin)) {
  case kCellI64: *w0 = i64_image((int64_t)*w0); break;
  case kCellF64: *w0 = f64_image(*w0); break;
  default: *w0 ^= 0x8000000000000000ull; break; // Decimal128: the high word's sign
  }
}

__global__ __launch_bounds__(kOrderBlock) void order_key_kernel(OrderParams p) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += stride) {
    const uint64_t *g = p.lanes + i * (uint64_t)p.k;
    for (int e = 0; e < p.n_err; ++e)
      if (agg_finalize_fails(g, p.err_lane[e], p.err_count_lane[e])) atomicMin(p.first_bad + e, (unsigned long long)i);
    for (int j = 0; j < p.n_terms; ++j) {
      const OrderTerm &t = p.t[j];
      bool null;
      uint64_t w0, w1 = 0;
      if (t.kind == kTermAgg) agg_image(t.a, g, &null, &w0, &w1);
      else {
        null = !p.kvalid[(uint64_t)t.key * p.n + i];
        const int64_t v = p.kv[(uint64_t)t.key * p.n + i];
        w0 = null ? 0 : t.kind == kTermKeyUtf8 ? (uint64_t)t.rank[(uint64_t)v & 255u] : i64_image(v);
      }
      if (null) w0 = w1 = 0;
      else if (t.desc) { w0 = ~w0; w1 = ~w1; }
      const bool two = t.kind == kTermAgg && agg_cell_type((AggFinal)t.a.fin) == kCellDec;
      p.keys[(uint64_t)t.word * p.n + i] = null == (bool)t.nulls_first ? 0u : 1u;
      p.keys[(uint64_t)(t.word + 1) * p.n + i] = w0;
      if (two) p.keys[(uint64_t)(t.word + 2) * p.n + i] = w1;
    }
  }
}

__device__ inline uint64_t key_word(const uint64_t *keys, uint64_t n, int n_words, int j, uint64_t i) {
  return j == n_words ? i : keys[(uint64_t)j * n + i];
}

__global__ __launch_bounds__(kOrderBlock) void order_radix_pass(const uint64_t *keys, uint64_t n, int n_words, int w, int shift, SelectState *st,
                                                               unsigned int *hist, unsigned int *arrived) {
  __shared__ unsigned int h[256];
  __shared__ unsigned long long pre[kMaxWords + 1], msk[kMaxWords + 1];
  __shared__ uint32_t done;
  for (uint32_t b = threadIdx.x; b < 256; b += blockDim.x) h[b] = 0;
  for (int j = threadIdx.x; j <= w; j += blockDim.x) { pre[j] = st->prefix[j]; msk[j] = st->mask[j]; }
  if (threadIdx.x == 0) done = st->done;
  __syncthreads();
  if (done) return; // (the whole grid: the state is the previous launch's)
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    bool live = true;
    for (int j = 0; j <= w && live; ++j) live = (key_word(keys, n, n_words, j, i) & msk[j]) == pre[j];
    if (live) atomicAdd(&h[(key_word(keys, n, n_words, w, i) >> shift) & 255u], 1u);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < 256; b += blockDim.x)
    if (h[b]) atomicAdd(hist + b, h[b]);
  // last arriver (agent-scope release / acquire around one counter; the histogram is atomics, read back with sc1 loads)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x != 0) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (atomicAdd(arrived, 1u) != gridDim.x - 1) return;
  // the last workgroup to arrive: every histogram is in — the digit of the threshold
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long need = st->need;
  unsigned long long before = 0, c = 0;
  uint32_t b = 0;
  for (; b < 256; ++b) {
    c = __hip_atomic_load(hist + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (before + c >= need) break;
    before += c;
  }
  if (b == 256) st->done = 1; // (unreachable: the tied groups hold at least `need`)
  else {
    st->prefix[w] |= (unsigned long long)b << shift;
    st->mask[w] |= 255ull << shift;
    st->need = need - before;
    if (c == need - before) st->done = 1; // the whole bucket is taken: the threshold is final
  }
  for (uint32_t x = 0; x < 256; ++x) hist[x] = 0;
  *arrived = 0;
}

// groups whose composite key, under the mask, is at most the threshold: exactly m of them
__global__ __launch_bounds__(kOrderBlock) void order_select_kernel(const uint64_t *keys, uint64_t n, int n_words, const SelectState *st, uint32_t *cand,
                                                                   uint32_t cap, unsigned int *count) {
  __shared__ unsigned long long pre[kMaxWords + 1], msk[kMaxWords + 1];
  for (int j = threadIdx.x; j <= n_words; j += blockDim.x) { pre[j] = st->prefix[j]; msk[j] = st->mask[j]; }
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    bool take = true;
    for (int j = 0; j <= n_words; ++j) {
      const uint64_t a = key_word(keys, n, n_words, j, i) & msk[j];
      if (a != pre[j]) { take = a < pre[j]; break; }
    }
    if (take) {
      const unsigned int at = atomicAdd(count, 1u);
      if (at < cap) cand[at] = (uint32_t)i;
    }
  }
}

// output position of every survivor = survivors with a smaller composite key (keys are distinct: the position is the last word)
constexpr uint32_t kRankTile = 128; // survivors per LDS tile (own keys 34 KiB + tile 17 KiB at the most words)
__global__ __launch_bounds__(kOrderBlock) void order_rank_kernel(const uint64_t *keys, uint64_t n, int n_words, const uint32_t *cand, uint32_t m, uint32_t offset,
                                                                 uint32_t *out_rows) {
  __shared__ uint64_t own[(kMaxWords + 1) * kOrderBlock];
  __shared__ uint64_t tile[(kMaxWords + 1) * kRankTile];
  const uint32_t c = blockIdx.x * kOrderBlock + threadIdx.x;
  const uint32_t mine = c < m ? cand[c] : 0;
  for (int j = 0; j <= n_words; ++j) own[j * kOrderBlock + threadIdx.x] = key_word(keys, n, n_words, j, mine);
  uint32_t rank = 0;
  for (uint32_t t0 = 0; t0 < m; t0 += kRankTile) {
    __syncthreads();
    const uint32_t e = t0 + threadIdx.x;
    if (threadIdx.x < kRankTile && e < m) {
      const uint32_t other = cand[e];
      for (int j = 0; j <= n_words; ++j) tile[j * kRankTile + threadIdx.x] = key_word(keys, n, n_words, j, other);
    }
    __syncthreads();
    const uint32_t in_tile = m - t0 < kRankTile ? m - t0 : kRankTile;
    for (uint32_t x = 0; x < in_tile; ++x) {
      for (int j = 0; j <= n_words; ++j) {
        const uint64_t a = tile[j * kRankTile + x], b = own[j * kOrderBlock + threadIdx.x];
        if (a != b) { rank += a < b; break; }
      }
    }
  }
  if (c < m && rank >= offset && rank < m) out_rows[rank - offset] = mine;
}

__global__ __launch_bounds__(kOrderBlock) void order_gather_kernel(const uint64_t *lanes, const int64_t *kv, const uint8_t *kvalid, uint64_t n, int k, int n_keys,
                                                                   const uint32_t *rows, uint32_t n_out, uint64_t *o_lanes, int64_t *o_kv, uint8_t *o_kvalid) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_out) return;
  const uint64_t g = rows[r];
  if (g >= n) return;
  for (int j = 0; j < k; ++j) o_lanes[(uint64_t)r * k + j] = lanes[g * k + j];
  for (int j = 0; j < n_keys; ++j) {
    o_kv[(uint64_t)j * n_out + r] = kv[(uint64_t)j * n + g];
    o_kvalid[(uint64_t)j * n_out + r] = kvalid[(uint64_t)j * n + g];
  }
}

bool is_decimal_fin(AggFinal f) { return agg_cell_type(f) == kCellDec; }

} // namespace

bool group_order_device_ok(const GroupOrderSpec &o, const LazyGroups &lz, std::string *why) {
  const uint64_t want = o.limit > UINT64_MAX - o.offset ? UINT64_MAX : o.offset + o.limit;
  if (want > kGroupOrderDeviceRows) { *why = "offset + limit above " + std::to_string(kGroupOrderDeviceRows); return false; }
  if (o.terms.size() > (size_t)kMaxTerms) { *why = "more than " + std::to_string(kMaxTerms) + " terms"; return false; }
  if (lz.n >= (1ull << 32)) { *why = "2^32 groups or more"; return false; }
  int words = 0, n_err = 0;
  for (const AggOut &a : lz.plan->aggs) n_err += agg_finalize_can_fail(a.fin);
  if (n_err > kMaxErrAggs) { *why = "more than " + std::to_string(kMaxErrAggs) + " i64 SUM / AVG aggregates"; return false; }
  for (const llkv_group_order_key &t : o.terms) {
    if (t.kind == LLKV_GROUP_ORDER_KEY) {
      const ColumnInfo *ci = lz.key_cols[t.index];
      words += 2;
      continue;
    }
    const AggOut &a = lz.plan->aggs[t.index];
    if (a.digits_lane >= 0) { *why = "aggregate " + std::to_string(t.index) + ": a computed DECIMAL argument"; return false; }
    words += is_decimal_fin(a.fin) ? 3 : 2;
  }
  if (words > kMaxWords) { *why = "more than " + std::to_string(kMaxWords) + " order-key words"; return false; }
  return true;
}

int group_order_device(const GroupOrderSpec &o, const LazyGroups &lz, const uint64_t *d_lanes, const int64_t *d_kv, const uint8_t *d_kvalid,
                       uint64_t n, hipStream_t s, GroupResultBuffers *h, uint64_t *n_out) {
  *n_out = 0;
  if (n == 0) return LLKV_OK;
  int rc;
  const LoweredPlan &plan = *lz.plan;
  const int K = lz.k;
  const uint32_t n_keys = lz.n_keys;
  OrderParams p;
  std::memset(&p, 0, sizeof p);
  p.lanes = d_lanes;
  p.kv = d_kv;
  p.kvalid = d_kvalid;
  p.n = n;
  p.k = K;
  std::vector<int> err_agg;
  for (size_t a = 0; a < plan.aggs.size(); ++a) {
    const AggOut &ao = plan.aggs[a];
    if (!agg_finalize_can_fail(ao.fin)) continue;
    p.err_lane[err_agg.size()] = ao.lane;
    p.err_count_lane[err_agg.size()] = ao.count_lane;
    err_agg.push_back((int)a);
  }
  p.n_err = (int32_t)err_agg.size();
  // Utf8 key terms: dictionary code → rank in byte order
  std::vector<uint32_t> ranks((size_t)std::max<size_t>(1, o.terms.size()) * 256, 0);
  int words = 0;
  for (size_t j = 0; j < o.terms.size(); ++j) {
    const llkv_group_order_key &k = o.terms[j];
    OrderTerm &t = p.t[j];
    t.word = words;
    t.desc = k.descending != 0;
    t.nulls_first = k.nulls_first != 0;
    if (k.kind == LLKV_GROUP_ORDER_KEY) {
      const ColumnInfo *ci = lz.key_cols[k.index];
      t.key = (int32_t)k.index;
      t.kind = ci->dtype == LLKV_DT_UTF8 && !utf8_wide(*ci) ? kTermKeyUtf8 : kTermKeyInt; // (a wide key's code is in byte order: its integer image)
      const std::vector<uint32_t> by_string = dictionary_ranks(*ci);
      std::copy(by_string.begin(), by_string.end(), ranks.begin() + j * 256);
      words += 2;
      continue;
    }
    const AggOut &a = plan.aggs[k.index];
    t.kind = kTermAgg;
    agg_cell_of(a, &t.a);
    words += is_decimal_fin(a.fin) ? 3 : 2;
  }
  p.n_terms = (int32_t)o.terms.size();
  p.n_words = words;
  const uint64_t m = o.end(n);
  const uint64_t rows_out = m > o.offset ? m - o.offset : 0;

  // one upload: rank tables, the select state, the error records, the histogram and its arrival counter
  SelectState st;
  std::memset(&st, 0, sizeof st);
  st.need = m;
  if (m >= n) st.done = 1; // every group: mask 0 selects them all
  for (int j = 0; j < words; ++j) st.mask[j] = 0;
  for (size_t j = 0; j < o.terms.size(); ++j) st.mask[p.t[j].word] = ~0xFFull; // NULL words: only the low byte varies
  {
    uint32_t nb = 1;
    while (nb < 8 && ((n - 1) >> (8 * nb)) != 0) ++nb;
    st.mask[words] = nb == 8 ? 0 : ~0ull << (8 * nb);
  }
  const size_t ranks_bytes = ranks.size() * 4, st_off = (ranks_bytes + 15) & ~(size_t)15, bad_off = st_off + sizeof(SelectState),
               hist_off = bad_off + (size_t)kMaxErrAggs * 8, total = hist_off + 257 * 4;
  std::vector<uint8_t> blob(total, 0);
  std::memcpy(blob.data(), ranks.data(), ranks_bytes);
  std::memcpy(blob.data() + st_off, &st, sizeof st);
  std::memset(blob.data() + bad_off, 0xFF, (size_t)kMaxErrAggs * 8);
  Scratch meta, keys, cand, rows, count, o_lanes, o_kv, o_kvalid;
  if ((rc = meta.alloc(total)) || (words && (rc = keys.alloc((size_t)words * n * 8)))) return rc;
  HIP_TRY(hipMemcpyAsync(meta.p, blob.data(), total, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s)); // `blob` is a local
  uint8_t *mb = meta.as<uint8_t>();
  SelectState *d_st = reinterpret_cast<SelectState *>(mb + st_off);
  unsigned int *d_hist = reinterpret_cast<unsigned int *>(mb + hist_off), *d_arrived = d_hist + 256;
  for (size_t j = 0; j < o.terms.size(); ++j) p.t[j].rank = reinterpret_cast<const uint32_t *>(mb) + j * 256;
  p.keys = keys.as<uint64_t>();
  p.first_bad = reinterpret_cast<unsigned long long *>(mb + bad_off);

  if (words || p.n_err) {
    hipLaunchKernelGGL(order_key_kernel, dim3(grid_for(n)), dim3(kOrderBlock), 0, s, p);
    HIP_TRY(hipGetLastError());
  }
  if (p.n_err) { // the first failing group of the first aggregate that has one: the host's finalize words the error
    uint64_t bad[kMaxErrAggs];
    Readback rb;
    if ((rc = rb.add(bad, p.first_bad, (size_t)p.n_err * 8, s)) || (rc = rb.wait())) return rc;
    for (int e = 0; e < p.n_err; ++e) {
      if (bad[e] == ~0ull) continue;
      return group_finalize_failure(plan, err_agg[(size_t)e], d_lanes, bad[e], K, s);
    }
  }
  if (rows_out == 0) return LLKV_OK;
  const uint32_t grid = grid_for(n);
  if (m < n) {
    for (int w = 0; w <= words; ++w) {
      for (int b = 7; b >= 0; --b) {
        if ((st.mask[w] >> (8 * b)) & 0xFF) continue; // a byte known to be zero
        hipLaunchKernelGGL(order_radix_pass, dim3(grid), dim3(kOrderBlock), 0, s, (const uint64_t *)p.keys, n, words, w, 8 * b, d_st, d_hist, d_arrived);
        HIP_TRY(hipGetLastError());
      }
    }
  }
  if ((rc = cand.alloc(m * 4)) || (rc = count.alloc(4)) || (rc = rows.alloc(rows_out * 4)) || (rc = o_lanes.alloc(rows_out * (size_t)K * 8)) ||
      (rc = o_kv.alloc(rows_out * n_keys * 8 + 8)) || (rc = o_kvalid.alloc(rows_out * n_keys + 8)))
    return rc;
  HIP_TRY(hipMemsetAsync(count.p, 0, 4, s));
  hipLaunchKernelGGL(order_select_kernel, dim3(grid), dim3(kOrderBlock), 0, s, (const uint64_t *)p.keys, n, words, (const SelectState *)d_st, cand.as<uint32_t>(),
                     (uint32_t)m, count.as<unsigned int>());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(order_rank_kernel, dim3((uint32_t)((m + kOrderBlock - 1) / kOrderBlock)), dim3(kOrderBlock), 0, s, (const uint64_t *)p.keys, n, words,
                     (const uint32_t *)cand.as<uint32_t>(), (uint32_t)m, (uint32_t)o.offset, rows.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(order_gather_kernel, dim3((uint32_t)((rows_out + kOrderBlock - 1) / kOrderBlock)), dim3(kOrderBlock), 0, s, d_lanes, d_kv, d_kvalid, n, K,
                     (int)n_keys, (const uint32_t *)rows.as<uint32_t>(), (uint32_t)rows_out, o_lanes.as<uint64_t>(), o_kv.as<int64_t>(), o_kvalid.as<uint8_t>());
  HIP_TRY(hipGetLastError());
  if ((rc = h->reserve(rows_out * (size_t)K * 8, rows_out * n_keys * 8 + 8, rows_out * n_keys + 8))) return rc;
  uint32_t selected = 0;
  HIP_TRY(hipMemcpyAsync(h->lanes.p, o_lanes.p, rows_out * (size_t)K * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(h->kv.p, o_kv.p, rows_out * n_keys * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(h->kvalid.p, o_kvalid.p, rows_out * n_keys, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&selected, count.p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (selected != m) return set_error(LLKV_INTERNAL, "device top-k selected " + std::to_string(selected) + " groups, not " + std::to_string(m));
  *n_out = rows_out;
  return LLKV_OK;
}

int group_finalize_failure(const LoweredPlan &plan, int agg, const uint64_t *d_lanes, uint64_t group, int k, hipStream_t s) {
  std::vector<uint64_t> g((size_t)k);
  HIP_TRY(hipMemcpyAsync(g.data(), d_lanes + group * (uint64_t)k, (size_t)k * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  llkv_value v;
  std::string err;
  if (int rc = finalize_value(plan.aggs[(size_t)agg], g.data(), 2, &v, &err, false)) return set_error(rc, err);
  return set_error(LLKV_INTERNAL, "device finalize check disagrees with the host's for aggregate " + std::to_string(agg));
}

// ---- host order ----------------------------------------------------------------------------------------------------------
int group_order_host(const GroupOrderSpec &o, uint64_t n, const std::function<int(uint64_t, const llkv_group_order_key &, llkv_value *)> &cell,
                     std::vector<uint64_t> *rows) {
  rows->clear();
  const uint64_t m = o.end(n);
  const size_t T = o.terms.size(), W = 3 * T; // per term: NULL word, two value words
  std::vector<uint64_t> img((size_t)n * W, 0);
  std::vector<llkv_value> col((size_t)n);
  for (size_t j = 0; j < T; ++j) {
    const llkv_group_order_key &t = o.terms[j];
    int rc;
    for (uint64_t r = 0; r < n; ++r)
      if ((rc = cell(r, t, &col[r]))) return rc;
    std::vector<uint64_t> str_rank;
    bool any_str = false;
    for (uint64_t r = 0; r < n && !any_str; ++r) any_str = !col[r].is_null && col[r].dtype == LLKV_DT_UTF8;
    if (any_str) { // strings by their bytes (str::cmp)
      std::vector<uint64_t> idx;
      for (uint64_t r = 0; r < n; ++r) if (!col[r].is_null) idx.push_back(r);
      auto str = [&](uint64_t r) { return col[r].str ? col[r].str : ""; };
      std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return std::strcmp(str(a), str(b)) < 0; });
      str_rank.assign((size_t)n, 0);
      for (size_t x = 1; x < idx.size(); ++x) str_rank[idx[x]] = str_rank[idx[x - 1]] + (std::strcmp(str(idx[x - 1]), str(idx[x])) != 0);
    }
    for (uint64_t r = 0; r < n; ++r) {
      const llkv_value &v = col[r];
      uint64_t *w = img.data() + (size_t)r * W + 3 * j;
      const bool null = v.is_null != 0;
      w[0] = null == (t.nulls_first != 0) ? 0 : 1;
      if (null) continue;
      switch (v.dtype) {
      case LLKV_DT_FLOAT64: { uint64_t b; std::memcpy(&b, &v.f64, 8); w[1] = (b >> 63) ? ~b : (b | 0x8000000000000000ull); break; }
      case LLKV_DT_DECIMAL128: w[1] = (uint64_t)v.i64_hi ^ 0x8000000000000000ull; w[2] = (uint64_t)v.i64; break;
      case LLKV_DT_UTF8: w[1] = str_rank[r]; break;
      default: w[1] = (uint64_t)v.i64 ^ 0x8000000000000000ull; break;
      }
      if (t.descending) { w[1] = ~w[1]; w[2] = ~w[2]; }
    }
  }
  std::vector<uint64_t> idx((size_t)n);
  std::iota(idx.begin(), idx.end(), 0ull);
  auto before = [&](uint64_t a, uint64_t b) {
    const uint64_t *x = img.data() + (size_t)a * W, *y = img.data() + (size_t)b * W;
    for (size_t j = 0; j < W; ++j)
      if (x[j] != y[j]) return x[j] < y[j];
    return a < b; // ties: position in the unordered output
  };
  if (m < n) std::partial_sort(idx.begin(), idx.begin() + (ptrdiff_t)m, idx.end(), before);
  else std::sort(idx.begin(), idx.end(), before);
  if (m > o.offset) rows->assign(idx.begin() + (ptrdiff_t)o.offset, idx.begin() + (ptrdiff_t)m);
  return LLKV_OK;
}

} // namespace llkv
