// scan_topn.hip — llkv_hip_scan_topn: ORDER BY projected columns, then OFFSET / LIMIT, over the selected rows of a projection scan
// (needs_post_sort llkv-executor/src/lib.rs:10979-11130 → sort_record_batch_with_order :13762-13868, SelectExecution::stream
// :10918-10955: arrow's lexsort over every selected row, then the slice).  Only the rows returned leave HBM.
//
//   selection    run_selection        the selected rows in scan order: positions and device rows (stream.cpp)
//   select       topn_radix_pass      exact radix select of the first m = offset + limit rows over the composite key (per term a NULL
//                                     word when the column has a validity mask, and a value word; then the selection index = the tie
//                                     break).  The words are never stored: every pass reads the cells of the staged columns through
//                                     the selection's device rows and forms the image in registers.  One 8-bit digit per launch, a
//                                     histogram of the rows still tied with the threshold, the last workgroup to arrive moves the
//                                     threshold (group_order.hip: order_radix_pass — same fences, atomics and resets).  Only the bytes
//                                     a word can vary in are visited: the value range of a signed column with statistics, the code
//                                     width of a Utf8 column, 1 for Boolean and NULL words, the bytes of n − 1 for the index.
//                topn_select_kernel   the m rows at or below the threshold
//   rank         topn_keys_kernel     the survivors' words, [word][m]
//                topn_rank_kernel     each survivor counts the survivors below it (16 survivors per workgroup, the others split over its
//                                     threads): its output position; rows [offset, m) leave as device rows and row ids
//   gather       the Project kernel of scan_stream, once over those device rows → one batch of at most kGroupOrderDeviceRows rows
// A candidate cut (the rows at or below the first term's threshold compacted into a list for the later passes) was built and
// measured, and removed: profiles/scan_topn/README.md.
#include "engine.hpp"
#include "order_select.hip.h"

#include <cstring>
#include <vector>

namespace llkv {

namespace {

enum TopnKind : int32_t { kTopnSigned = 0, kTopnUnsigned = 1, kTopnBool = 2, kTopnF64 = 3, kTopnF32 = 4, kTopnRank = 5 };

struct TopnTerm {
  const void *values;
  const uint8_t *valid;    // 1 B/row validity mask, nullptr: the column has no NULL cell (and the term no NULL word)
  const uint32_t *rank;    // kTopnRank: 1-byte dictionary code → position of its string in byte order
  unsigned long long base; // integers and ranks: image = v − base, DESC: base − v
  int32_t width, kind, desc, nulls_first;
};

struct TopnParams {
  const uint64_t *dev; // selection index → device row
  uint64_t n;
  int32_t n_words;     // words of the terms; word n_words is the selection index
  int8_t word_term[kMaxWords], word_null[kMaxWords];
  TopnTerm t[kMaxTerms];
};

// The passes stream the whole selection: workgroups of 1 024 threads, two per CU — a quarter of the workgroups a 256-thread launch
// would need for the same threads in flight, and so a quarter of the adds into the global histogram, which all land on 256 addresses
// (2 048 workgroups spent 50 µs per pass on them whatever the row count).  A small selection gets four rows per thread for the same reason.
constexpr uint32_t kTopnBlock = 1024;
uint32_t topn_grid(uint64_t n) {
  const uint64_t want = (n + 4 * kTopnBlock - 1) / (4 * kTopnBlock), cap = (uint64_t)g_ctx.cu_count * 2;
  return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}

// word j of the composite key of selection index i (device row `dev`); an invalid cell's value is never read
__device__ inline uint64_t topn_word(const TopnParams &p, int j, uint64_t i, uint64_t dev) {
  if (j == p.n_words) return i;
  const TopnTerm &t = p.t[p.word_term[j]];
  const bool null = t.valid && !t.valid[dev];
  if (p.word_null[j]) return null == (bool)t.nulls_first ? 0u : 1u;
  if (null) return 0;
  const uint64_t raw = t.width == 8 ? static_cast<const uint64_t *>(t.values)[dev]
                     : t.width == 4 ? (uint64_t) static_cast<const uint32_t *>(t.values)[dev]
                                    : (uint64_t) static_cast<const uint8_t *>(t.values)[dev];
  switch (t.kind) {
  case kTopnSigned: {
    const uint64_t v = t.width == 8 ? raw : (uint64_t)(int64_t)(int32_t)raw;
    return t.desc ? t.base - v : v - t.base;
  }
  case kTopnUnsigned: return t.desc ? t.base - raw : raw - t.base;
  case kTopnBool: return (raw != 0) != (t.desc != 0) ? 1u : 0u;
  case kTopnF64: return t.desc ? ~f64_image(raw) : f64_image(raw);
  case kTopnF32: {
    const uint32_t b = (uint32_t)raw, img = (b >> 31) ? ~b : (b | 0x80000000u); // f32::total_cmp
    return t.desc ? (uint32_t)~img : img;
  }
  default: {
    const uint64_t r = t.rank[raw & 255u];
    return t.desc ? t.base - r : r;
  }
  }
}

__global__ __launch_bounds__(kTopnBlock) void topn_radix_pass(TopnParams p, int w, int shift, SelectState *st, unsigned int *hist, unsigned int *arrived) {
  __shared__ unsigned int h[256];
  __shared__ unsigned long long pre[kMaxWords + 1], msk[kMaxWords + 1];
  __shared__ uint32_t done, last;
  for (uint32_t b = threadIdx.x; b < 256; b += blockDim.x) h[b] = 0;
  for (int j = threadIdx.x; j <= w; j += blockDim.x) { pre[j] = st->prefix[j]; msk[j] = st->mask[j]; }
  if (threadIdx.x == 0) done = st->done;
  __syncthreads();
  if (done) return; // (the whole grid: the state is the previous launch's)
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t rounds = (p.n + stride - 1) / stride; // every lane of a wave makes every round: the digits are counted per wave
  for (uint64_t r = 0; r < rounds; ++r) {
    const uint64_t i = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool live = i < p.n;
    uint32_t digit = 0;
    if (live) {
      const uint64_t dev = p.dev[i];
      for (int j = 0; j < w && live; ++j) live = (topn_word(p, j, i, dev) & msk[j]) == pre[j]; // a row that left the tie at an earlier word stops there
      if (live) {
        const uint64_t word = topn_word(p, w, i, dev);
        live = (word & msk[w]) == pre[w];
        digit = (uint32_t)(word >> shift) & 255u;
      }
    }
    // Few distinct digits in a wave are the rule (a 3-valued column, the upper bytes of neighbouring indices): 64 adds to one LDS
    // address serialise, so up to four digits are counted with a ballot and added once; whoever is left adds for itself.
    uint64_t todo = __ballot(live);
    for (int k = 0; k < 4 && todo; ++k) {
      const uint32_t d = (uint32_t)__shfl((int)digit, __ffsll((unsigned long long)todo) - 1);
      const uint64_t same = __ballot(live && digit == d);
      if ((threadIdx.x & 63u) == (uint32_t)(__ffsll((unsigned long long)todo) - 1)) atomicAdd(&h[d], (unsigned int)__popcll(same));
      if (live && digit == d) live = false;
      todo &= ~same;
    }
    if (live) atomicAdd(&h[digit], 1u);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < 256; b += blockDim.x)
    if (h[b]) atomicAdd(hist + b, h[b]);
  // last arriver (agent-scope release / acquire around one counter; the histogram is atomics, read back with sc1 loads): the fences,
  // the waits and the ticket are order_radix_pass's, by one lane; what differs is who reads the histogram afterwards — the whole
  // workgroup, one bin per thread behind that lane's acquire and a barrier, instead of one thread walking 256 dependent loads
  // (up to 40 µs of a pass over 600 000 rows)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = atomicAdd(arrived, 1u) == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  // the last workgroup to arrive: every histogram is in — the digit of the threshold.  h[b] = rows in the bins up to b (fewer than 2^32 rows)
  const uint32_t b = threadIdx.x;
  const unsigned int c = b < 256 ? __hip_atomic_load(hist + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  const unsigned long long need = st->need; // (read by everybody before the barriers below, written behind them)
  if (b < 256) h[b] = c;
  __syncthreads();
  for (uint32_t step = 1; step < 256; step <<= 1) {
    const unsigned int add = b < 256 && b >= step ? h[b - step] : 0u;
    __syncthreads();
    if (b < 256) h[b] += add;
    __syncthreads();
  }
  if (b < 256) {
    const unsigned long long upto = h[b], before = upto - c;
    if (before < need && need <= upto) { // the one bin the need falls into
      st->prefix[w] |= (unsigned long long)b << shift;
      st->mask[w] |= 255ull << shift;
      st->need = need - before;
      if (c == need - before) st->done = 1; // the whole bucket is taken: the threshold is final
    }
    if (b == 255 && upto < need) st->done = 1; // (unreachable: the tied rows hold at least `need`)
    hist[b] = 0;
  }
  if (b == 0) *arrived = 0;
}

// rows whose composite key, under the mask, is at most the threshold: exactly m of them
__global__ __launch_bounds__(kTopnBlock) void topn_select_kernel(TopnParams p, const SelectState *st, uint32_t *cand, uint32_t cap, unsigned int *count) {
  __shared__ unsigned long long pre[kMaxWords + 1], msk[kMaxWords + 1];
  for (int j = threadIdx.x; j <= p.n_words; j += blockDim.x) { pre[j] = st->prefix[j]; msk[j] = st->mask[j]; }
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += stride) {
    const uint64_t dev = p.dev[i];
    bool take = true;
    for (int j = 0; j <= p.n_words; ++j) {
      const uint64_t a = topn_word(p, j, i, dev) & msk[j];
      if (a != pre[j]) { take = a < pre[j]; break; }
    }
    if (take) {
      const unsigned int at = atomicAdd(count, 1u);
      if (at < cap) cand[at] = (uint32_t)i;
    }
  }
}

// The survivors' words, [n_words + 1][m] (the last one is the selection index itself).  cand = nullptr: the survivors are the
// selection indices 0 … m − 1 (every selected row, or no term at all).
__global__ __launch_bounds__(kOrderBlock) void topn_keys_kernel(TopnParams p, const uint32_t *cand, uint32_t m, uint64_t *keys) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  uint32_t mine = cand ? cand[c] : c;
  if (mine >= p.n) mine = 0; // (a survivor list the host is about to refuse: stay inside the selection)
  const uint64_t dev = p.dev[mine];
  for (int j = 0; j <= p.n_words; ++j) keys[(uint64_t)j * m + c] = topn_word(p, j, mine, dev);
}

// Output position of every survivor = survivors with a smaller composite key (keys are distinct: the selection index is the last
// word).  A workgroup ranks kRankOwn survivors; its threads split all survivors 64 ways (the own words sit in LDS, a thread walks at
// most 16 others: the loop is a chain of load latencies, so it is kept short), the partial ranks meet in LDS.  Rows [offset, m) leave in order as
// device rows (what the Project kernel gathers) and as the row ids the batch reports.
constexpr uint32_t kRankOwn = 16, kRankBlock = 1024;
__global__ __launch_bounds__(kRankBlock) void topn_rank_kernel(const uint64_t *keys, int n_words, uint32_t m, uint32_t offset, const uint64_t *dev, const uint64_t *positions,
                                                               const uint64_t *table_ids, uint64_t *out_dev, uint64_t *out_ids) {
  __shared__ uint64_t own[(kMaxWords + 1) * kRankOwn];
  __shared__ unsigned int rank[kRankOwn];
  const uint32_t o = threadIdx.x & (kRankOwn - 1), part = threadIdx.x / kRankOwn, parts = kRankBlock / kRankOwn;
  const uint32_t c = blockIdx.x * kRankOwn + o;
  for (int j = (int)part; j <= n_words; j += (int)parts) own[j * kRankOwn + o] = c < m ? keys[(uint64_t)j * m + c] : 0;
  if (part == 0) rank[o] = 0;
  __syncthreads();
  const uint32_t chunk = (m + parts - 1) / parts, x0 = part * chunk, x1 = x0 + chunk < m ? x0 + chunk : m;
  unsigned int below = 0;
  for (uint32_t x = x0; x < x1; ++x) {
    bool less = false, equal = true; // the other's key < mine, decided by the first word that differs
    for (int j = 0; j <= n_words; ++j) {
      const uint64_t a = keys[(uint64_t)j * m + x], b = own[j * kRankOwn + o];
      less |= equal && a < b;
      equal &= a == b;
    }
    below += less;
  }
  if (below) atomicAdd(&rank[o], below);
  __syncthreads();
  if (part != 0 || c >= m) return;
  const uint32_t r = rank[o];
  if (r < offset || r >= m) return;
  uint64_t mine = own[n_words * kRankOwn + o]; // the selection index
  const uint64_t my_dev = dev[mine];
  out_dev[r - offset] = my_dev;
  if (out_ids) out_ids[r - offset] = table_ids ? table_ids[my_dev] : positions[mine];
}

uint32_t bytes_of(unsigned __int128 range) { // digits of 8 bits the values 0 … range need
  uint32_t b = 0;
  while (b < 8 && (range >> (8 * b)) != 0) ++b;
  return b;
}

// The term's descriptor and how many low bytes of its value word can vary.
uint32_t describe_term(const DeviceColumn &c, const llkv_scan_order_term &o, const uint32_t *d_rank, TopnTerm *t) {
  const ColumnInfo &ci = c.info;
  t->values = c.d_values.get();
  t->valid = ci.nullable ? c.d_valid.get<uint8_t>() : nullptr;
  t->rank = nullptr;
  t->base = 0;
  t->desc = o.descending != 0;
  t->nulls_first = o.nulls_first != 0;
  t->width = (int32_t)dtype_width(storage_dtype(ci));
  switch (storage_dtype(ci)) {
  case LLKV_DT_FLOAT64: t->kind = kTopnF64; return 8;
  case LLKV_DT_FLOAT32: t->kind = kTopnF32; return 4;
  case LLKV_DT_BOOLEAN: t->kind = kTopnBool; return 1;
  case LLKV_DT_UTF8: // 1-byte codes in first-appearance order: by the rank of their strings
    t->kind = kTopnRank;
    t->rank = d_rank;
    t->base = 255;
    return 1;
  case LLKV_DT_UINT64: case LLKV_DT_UINT32: { // (a wide Utf8 column's codes are in byte order: 0 … dictionary − 1)
    t->kind = kTopnUnsigned;
    const uint64_t top = utf8_wide(ci) ? (uint64_t)ci.dictionary.size() - 1 : t->width == 8 ? ~0ull : 0xFFFFFFFFull;
    if (t->desc) t->base = top;
    return bytes_of(top);
  }
  default: { // Int64, Int32, Date32, Decimal128 narrowed to 64 bits: v − min, DESC max − v — only the bytes the value range needs
    t->kind = kTopnSigned;
    const int64_t lo = ci.has_stats ? ci.min_i : t->width == 8 ? INT64_MIN : (int64_t)INT32_MIN;
    const int64_t hi = ci.has_stats ? ci.max_i : t->width == 8 ? INT64_MAX : (int64_t)INT32_MAX;
    t->base = (unsigned long long)(t->desc ? hi : lo);
    return bytes_of((unsigned __int128)((__int128)hi - (__int128)lo));
  }
  }
}

} // namespace

// The refusals that need no device, in the order llkv_hip_scan_topn has always made them (`world`: the table's, so that the sharded
// refusal keeps its place among them).
int topn_refusals(const llkv_scan_options *options, uint32_t n_projections, const llkv_scan_order_term *order, uint32_t n_order, uint64_t offset, uint64_t limit,
                  uint32_t world) {
  if (n_order && !order) return set_error(LLKV_INVALID_ARGUMENT, "NULL argument: " + std::to_string(n_order) + " ORDER BY terms without a term array");
  if (options && options->order_enabled)
    return set_error(LLKV_INVALID_ARGUMENT, "llkv_scan_options.order does not combine with the ORDER BY terms of llkv_hip_scan_topn: leave order_enabled 0");
  for (uint32_t j = 0; j < n_order; ++j)
    if (order[j].projection >= n_projections)
      return set_error(LLKV_INVALID_ARGUMENT, "ORDER BY position " + std::to_string((uint64_t)order[j].projection + 1) + " is out of bounds for " + std::to_string(n_projections) + " columns");
  if (world > 1) return set_error(LLKV_UNSUPPORTED, "scan top-N over a sharded table (world " + std::to_string(world) + "): order each rank's rows and merge them in the binding");
  if (n_order > (uint32_t)kMaxTerms) return set_error(LLKV_UNSUPPORTED, "scan top-N with " + std::to_string(n_order) + " ORDER BY terms: more than " + std::to_string(kMaxTerms) + " terms");
  if (limit > UINT64_MAX - offset || offset + limit > kGroupOrderDeviceRows)
    return set_error(LLKV_UNSUPPORTED, "scan top-N with offset + limit above " + std::to_string(kGroupOrderDeviceRows) + ": use llkv_hip_scan_stream");
  return LLKV_OK;
}

int scan_topn(const Table *t, const llkv_projection *projections, uint32_t n_projections, const llkv_filter *filters, uint32_t n_filters,
              const llkv_eval_op *ops, uint32_t n_ops, const llkv_scan_options *options, const llkv_scan_order_term *order, uint32_t n_order,
              uint64_t offset, uint64_t limit, llkv_on_batch on_batch, void *user, uint64_t *total_rows) {
  if (total_rows) *total_rows = 0;
  // refusals: before any device work
  if (!t || !on_batch) return set_error(LLKV_INVALID_ARGUMENT, "NULL argument: llkv_hip_scan_topn needs a table and an on_batch callback");
  int rc = topn_refusals(options, n_projections, order, n_order, offset, limit, t->world);
  if (rc) return rc;
  for (uint32_t i = 0; i < n_projections; ++i)
    if (projections[i].computed)
      return set_error(LLKV_UNSUPPORTED, "scan top-N with a computed projection (projection " + std::to_string(i) + "): its arithmetic errors in rows that are not returned must still fail the query");
  if ((rc = ensure_device())) return rc;
  LoweredPlan proj;
  std::string err;
  if ((rc = lower_projection(table_resolver(*t), projections, n_projections, &proj, &err))) return set_error(rc, err);
  for (uint32_t j = 0; j < n_order; ++j) {
    const ColumnInfo &ci = t->cols.at(projections[order[j].projection].field_id).info;
    if (ci.wide128)
      return set_error(LLKV_UNSUPPORTED, "scan top-N by field " + std::to_string(ci.field_id) + ": a Decimal128 column staged beyond 64 bits");
  }
  // the selection scan_stream makes: include_nulls = false drops the rows whose projected cells are all NULL
  std::vector<uint32_t> gathered;
  if (!(options && options->include_nulls))
    for (uint32_t i = 0; i < n_projections; ++i) gathered.push_back(projections[i].field_id);
  Selection sel;
  if ((rc = run_selection(t, filters, n_filters, ops, n_ops, &sel, gathered.data(), (uint32_t)gathered.size()))) return rc;
  if (total_rows) *total_rows = sel.n;
  return topn_over_selection(t, proj, projections, options, order, n_order, offset, limit, sel, on_batch, user);
}

// Select, rank and gather over a selection in scan order (sel.d_ids: positions): rows [offset, offset + limit) of its order by the
// terms, in one callback; none when no row is left.
int topn_over_selection(const Table *t, const LoweredPlan &proj, const llkv_projection *projections, const llkv_scan_options *options,
                        const llkv_scan_order_term *order, uint32_t n_order, uint64_t offset, uint64_t limit, const Selection &sel, llkv_on_batch on_batch, void *user) {
  int rc;
  std::string err;
  const uint64_t n = sel.n;
  if (n >= (1ull << 32)) return set_error(LLKV_UNSUPPORTED, "scan top-N over 2^32 selected rows or more");
  const uint64_t m = std::min<uint64_t>(offset + limit, n);
  if (m <= offset) return LLKV_OK; // nothing left: no batch
  const uint32_t rows_out = (uint32_t)(m - offset);
  const bool with_ids = options && options->include_row_ids;
  hipStream_t s = g_ctx.stream;
  JitKernel k;
  if ((rc = jit_compile(JitKind::Project, proj.type_string, &k, &err))) return set_error(rc, err);

  // the composite key: per term a NULL word (columns with a validity mask) and a value word, then the selection index
  TopnParams p;
  std::memset(&p, 0, sizeof p);
  p.dev = sel.d_dev;
  p.n = n;
  uint32_t word_bytes[kMaxWords + 1];
  std::vector<uint32_t> ranks((size_t)std::max<uint32_t>(1, n_order) * 256, 0);
  const size_t ranks_bytes = ranks.size() * 4, st_off = (ranks_bytes + 15) & ~(size_t)15, hist_off = st_off + sizeof(SelectState), total = hist_off + 258 * 4;
  Scratch meta;
  if ((rc = meta.alloc(total))) return rc;
  uint8_t *mb = meta.as<uint8_t>();
  int words = 0;
  for (uint32_t j = 0; j < n_order; ++j) {
    const DeviceColumn &c = t->cols.at(projections[order[j].projection].field_id);
    const std::vector<uint32_t> by_string = dictionary_ranks(c.info);
    std::copy(by_string.begin(), by_string.end(), ranks.begin() + (size_t)j * 256);
    const uint32_t value_bytes = describe_term(c, order[j], reinterpret_cast<const uint32_t *>(mb) + (size_t)j * 256, &p.t[j]);
    if (p.t[j].valid) {
      p.word_term[words] = (int8_t)j;
      p.word_null[words] = 1;
      word_bytes[words++] = 1;
    }
    p.word_term[words] = (int8_t)j;
    word_bytes[words++] = value_bytes;
  }
  p.n_words = words;
  word_bytes[words] = bytes_of(n - 1);
  const bool select = m < n && words > 0; // else the survivors are the first m selected rows

  Scratch cand, keys, ord_dev, ord_ids, d_out[kMaxOuts], d_valid[kMaxOuts], d_err;
  PinnedBuf h_meta, h_out[kMaxOuts], h_valid[kMaxOuts], h_ids, h_tail;
  const uint32_t n_out = (uint32_t)proj.out_dtypes.size();
  auto out_width = [&](uint32_t o) -> size_t { return proj.out_wide[o] ? 4 : dtype_out_width(proj.out_dtypes[o]); }; // (wide Utf8: u32 codes)
  const size_t valid_bytes = (size_t)((rows_out + 63) / 64) * 8;
  if ((rc = keys.alloc((size_t)(words + 1) * m * 8)) || (rc = ord_dev.alloc((size_t)rows_out * 8)) || (rc = d_err.alloc(4)) || (rc = h_tail.alloc(8))) return rc;
  if (with_ids && ((rc = ord_ids.alloc((size_t)rows_out * 8)) || (rc = h_ids.alloc((size_t)rows_out * 8)))) return rc;
  for (uint32_t o = 0; o < n_out; ++o) {
    if ((rc = d_out[o].alloc((size_t)rows_out * out_width(o))) || (rc = h_out[o].alloc((size_t)rows_out * out_width(o)))) return rc;
    if (proj.out_nullable[o] && ((rc = d_valid[o].alloc(valid_bytes)) || (rc = h_valid[o].alloc(valid_bytes)))) return rc;
  }
  // from here on the stream runs ahead of the host: everything is waited for before the buffers go back to their pools
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{s};
  unsigned int *d_count = reinterpret_cast<unsigned int *>(mb + hist_off) + 257;
  if (select) {
    // one upload from pinned memory: rank tables, the select state, the zeroed histogram, its arrival counter and the survivor count
    SelectState st;
    std::memset(&st, 0, sizeof st);
    st.need = m;
    for (int j = 0; j <= words; ++j) st.mask[j] = word_bytes[j] >= 8 ? 0 : ~0ull << (8 * word_bytes[j]); // bytes known to be zero
    if ((rc = h_meta.alloc(total)) || (rc = cand.alloc((size_t)m * 4))) return rc;
    std::memset(h_meta.p, 0, total);
    std::memcpy(h_meta.p, ranks.data(), ranks_bytes);
    std::memcpy(static_cast<uint8_t *>(h_meta.p) + st_off, &st, sizeof st);
    HIP_TRY(hipMemcpyAsync(meta.p, h_meta.p, total, hipMemcpyHostToDevice, s));
    SelectState *d_st = reinterpret_cast<SelectState *>(mb + st_off);
    unsigned int *d_hist = reinterpret_cast<unsigned int *>(mb + hist_off), *d_arrived = d_hist + 256;
    const uint32_t grid = topn_grid(n);
    for (int w = 0; w <= words; ++w)
      for (int b = (int)word_bytes[w] - 1; b >= 0; --b) {
        hipLaunchKernelGGL(topn_radix_pass, dim3(grid), dim3(kTopnBlock), 0, s, p, w, 8 * b, d_st, d_hist, d_arrived);
        HIP_TRY(hipGetLastError());
      }
    hipLaunchKernelGGL(topn_select_kernel, dim3(grid), dim3(kTopnBlock), 0, s, p, (const SelectState *)d_st, cand.as<uint32_t>(), (uint32_t)m, d_count);
    HIP_TRY(hipGetLastError());
  } else if (words) { // every selected row is a survivor: only the rank tables are needed
    if ((rc = h_meta.alloc(ranks_bytes))) return rc;
    std::memcpy(h_meta.p, ranks.data(), ranks_bytes);
    HIP_TRY(hipMemcpyAsync(meta.p, h_meta.p, ranks_bytes, hipMemcpyHostToDevice, s));
  }
  hipLaunchKernelGGL(topn_keys_kernel, dim3((uint32_t)((m + kOrderBlock - 1) / kOrderBlock)), dim3(kOrderBlock), 0, s, p, select ? (const uint32_t *)cand.as<uint32_t>() : nullptr,
                     (uint32_t)m, keys.as<uint64_t>());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(topn_rank_kernel, dim3((uint32_t)((m + kRankOwn - 1) / kRankOwn)), dim3(kRankBlock), 0, s, (const uint64_t *)keys.as<uint64_t>(), words, (uint32_t)m,
                     (uint32_t)offset, (const uint64_t *)sel.d_dev, (const uint64_t *)sel.d_ids, t->d_row_ids ? t->d_row_ids.get<const uint64_t>() : nullptr,
                     ord_dev.as<uint64_t>(), with_ids ? ord_ids.as<uint64_t>() : nullptr);
  HIP_TRY(hipGetLastError());

  ProjParams q;
  bind_plan(proj, *t, &q);
  q.dev_rows = ord_dev.as<uint64_t>();
  q.n = rows_out;
  for (uint32_t o = 0; o < n_out; ++o) { q.out[o] = d_out[o].p; q.out_valid[o] = (uint64_t *)d_valid[o].p; }
  q.error_flag = d_err.as<uint32_t>();
  HIP_TRY(hipMemsetAsync(d_err.p, 0, 4, s));
  if ((rc = jit_launch_raw(k.fn, (rows_out + kBlock - 1) / kBlock, &q, sizeof q, s))) return rc;
  for (uint32_t o = 0; o < n_out; ++o) {
    HIP_TRY(hipMemcpyAsync(h_out[o].p, d_out[o].p, (size_t)rows_out * out_width(o), hipMemcpyDeviceToHost, s));
    if (proj.out_nullable[o]) HIP_TRY(hipMemcpyAsync(h_valid[o].p, d_valid[o].p, valid_bytes, hipMemcpyDeviceToHost, s));
  }
  if (with_ids) HIP_TRY(hipMemcpyAsync(h_ids.p, ord_ids.p, (size_t)rows_out * 8, hipMemcpyDeviceToHost, s));
  uint32_t *tail = static_cast<uint32_t *>(h_tail.p); // [0] the Project kernel's error cell, [1] the survivor count
  tail[1] = (uint32_t)m;
  HIP_TRY(hipMemcpyAsync(tail, d_err.p, 4, hipMemcpyDeviceToHost, s));
  if (select) HIP_TRY(hipMemcpyAsync(tail + 1, d_count, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (tail[1] != m) return set_error(LLKV_INTERNAL, "device top-N selected " + std::to_string(tail[1]) + " rows, not " + std::to_string(m));
  if (tail[0]) return set_error(LLKV_INTERNAL, arith_error_message(tail[0]));

  std::vector<std::vector<const char *>> dicts(n_out); // dictionaries of the Utf8 columns
  llkv_column_view cols[kMaxOuts];
  for (uint32_t o = 0; o < n_out; ++o) {
    const ColumnInfo &ci = t->cols.at((uint32_t)proj.out_fields[o]).info;
    if (proj.out_dtypes[o] == LLKV_DT_UTF8)
      for (auto &str : ci.dictionary) dicts[o].push_back(str.c_str());
    cols[o].dtype = proj.out_dtypes[o];
    cols[o].values = h_out[o].p;
    cols[o].validity = proj.out_nullable[o] ? (const uint8_t *)h_valid[o].p : nullptr;
    cols[o].dictionary = dicts[o].empty() ? nullptr : dicts[o].data();
    cols[o].precision = cols[o].scale = 0;
    if (proj.out_wide[o]) cols[o].precision = 4; // u32 codes of a wide Utf8 column
    if (proj.out_dtypes[o] == LLKV_DT_DECIMAL128) {
      cols[o].precision = ci.precision;
      cols[o].scale = ci.scale;
    }
  }
  llkv_batch_view b;
  b.num_rows = rows_out;
  b.num_columns = n_out;
  b.columns = cols;
  b.row_ids = with_ids ? (const uint64_t *)h_ids.p : nullptr;
  on_batch(&b, user); // calling thread, the one batch
  return LLKV_OK;
}

} // namespace llkv

extern "C" llkv_status llkv_hip_scan_topn(const llkv_hip_table *table, const llkv_projection *projections, uint32_t n_projections, const llkv_filter *filters,
                                          uint32_t n_filters, const llkv_eval_op *ops, uint32_t n_ops, const llkv_scan_options *options,
                                          const llkv_scan_order_term *order, uint32_t n_order, uint64_t offset, uint64_t limit, llkv_on_batch on_batch, void *user,
                                          uint64_t *total_rows) {
  return (llkv_status)llkv::scan_topn(reinterpret_cast<const llkv::Table *>(table), projections, n_projections, filters, n_filters, ops, n_ops, options, order, n_order,
                                      offset, limit, on_batch, user, total_rows);
}
