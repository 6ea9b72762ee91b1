// scan_distinct.hip — llkv_hip_scan_distinct: SELECT DISTINCT over the selected rows of a projection scan, deduplicated in HBM
// (the DISTINCT step of SelectExecution, llkv-executor/src/lib.rs:10984-11011 → distinct_filter_batch :13720-13760 over
// CanonicalRow, llkv-types/src/canonical.rs; then ORDER BY :11052-11067 and OFFSET / LIMIT, SelectExecution::stream :10918-10955;
// no NULL row is synthesised under DISTINCT, :11026 / :11039).  A row survives iff no earlier row of the scan has the same
// canonical row; the first occurrence leaves with its own cells.
//
//   selection   run_selection (+ sort_selection under options->order_enabled): the rows of scan_stream, in its order
//   key         per projected column one canonical 64-bit word and, for a column with a validity mask, a NULL flag — formed in
//               registers from the staged cells at the selection's device rows (dist_word), never stored for all rows.  Int64 /
//               Date32 / Decimal128 narrowed to 64 bits: the value; Boolean: 0 / 1; Float64: the bits, every NaN one pattern,
//               −0.0 as +0.0 (canonical.rs:140-147); Utf8: the dictionary code (every dictionary holds a string once: staging and
//               appends refuse a duplicate).  The bytes under an invalid cell are never read.
//   dedup       the smallest selection index of every class of equal rows, left in a table of uint32 cells (0xFFFFFFFF = none):
//     direct    distinct_direct_insert — the statistics bound every column (integer / date range, Boolean, dictionary size), so the
//               row IS a small mixed-radix integer (a nullable column has one more digit value, NULL = 0) and owns cell[key]:
//               atomicMin(cell[key], i) behind a relaxed load — a row whose index is not below the cell's value issues no atomic
//               (60 M rows of 4 classes would otherwise queue on 4 addresses), and the lanes of a wave that share a cell leave it to
//               the lowest of them.  A valid cell outside its column's statistics raises the error cell instead of leaving the table.
//     hash      distinct_hash_insert — everything else.  Open addressing, linear probing, a power-of-two capacity >= 2 n; a slot
//               holds the selection index of its class's representative.  Row i hashes its words and walks from its home slot:
//               an empty slot is claimed by compare-and-swap (empty → i); an occupied one is compared with row i over ALL
//               canonical words by reading the representative's cells (the hash never decides equality) — equal: atomicMin(slot, i)
//               when the slot's index is above i, then stop; different: the next slot.
//               Why the result is the minimum index of every class whatever the interleaving: a slot is never emptied, and the
//               class of the row it holds never changes (a claim writes into an empty slot only, the min only replaces a row by an
//               equal one).  So all rows of a class walk the same sequence of slots, pass the same foreign slots, and meet in the
//               first slot that any of them claimed: one slot per class.  That slot's value only decreases, and only to indices of
//               its class; every row of the class either claimed it or, having read a value v, issued the min unless v <= i.  A
//               stale read can only show an OLDER state — still empty (the CAS then fails and returns the row that is there) or a
//               larger index of the same class (one min that was not needed) — never a wrong skip and never a wrong claim.  The
//               table therefore ends the same for every launch geometry and timing.
//               Every slot access is an agent-scope atomic (relaxed load, CAS, min).  No thread waits for another: no flags, no
//               hand-off between workgroups.  A row gives up after `capacity` probes and raises the error cell (LLKV_INTERNAL): a
//               defect in the table ends the kernel instead of hanging the device.
//   survivors   distinct_mark — every occupied cell flags its row (and is counted: the count must equal the survivors');
//               an exclusive scan of the flags; distinct_compact gathers the flagged rows' device rows and positions, in
//               selection order, into a new Selection.  (The other form — compact the cells, sort them — is not built: see
//               profiles/scan_distinct/README.md.)
//   delivery    no ORDER BY term: rows [offset, offset + limit) of the survivors through deliver_windows (stream.cpp), as scan_stream
//               delivers; with terms: topn_over_selection (scan_topn.hip) over the survivors.
// LLKV_HIP_DISTINCT_ROUTE = direct | hash forces the route (a direct route the columns do not admit: LLKV_UNSUPPORTED);
// LLKV_HIP_DISTINCT_HASH_BITS = k keeps only the low k bits of the hash (long probe chains, same capacity).  Both are read at
// every call and change no result.
// The descriptor, dist_word, the hash, the two inserts and the compaction live in distinct_key.hip.h: llkv_hip_scan_setop
// (scan_setop.hip) runs them over two scans, with its own word for Float64.
#include "distinct_key.hip.h"

#include <cstring>
#include <vector>

namespace llkv {

namespace {

// Every occupied cell flags the row it names; the occupied cells are counted (one add per workgroup).
__global__ __launch_bounds__(kDistBlock) void distinct_mark(const uint32_t *table, uint64_t n_table, uint64_t n, uint64_t *flags, unsigned long long *occupied, uint32_t *error) {
  __shared__ unsigned int block_count;
  if (threadIdx.x == 0) block_count = 0;
  __syncthreads();
  unsigned int mine = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_table; c += stride) {
    const uint32_t v = table[c];
    if (v == kDistEmpty) continue;
    ++mine;
    if (v < n) flags[v] = 1;
    else atomicOr(error, (uint32_t)kDistErrIndex);
  }
  if (mine) atomicAdd(&block_count, mine);
  __syncthreads();
  if (threadIdx.x == 0 && block_count) atomicAdd(occupied, (unsigned long long)block_count);
}

const char *type_name(int32_t dtype) {
  switch (dtype) {
  case LLKV_DT_INT32: return "Int32";
  case LLKV_DT_UINT32: return "UInt32";
  case LLKV_DT_UINT64: return "UInt64";
  case LLKV_DT_FLOAT32: return "Float32";
  default: return nullptr; // a type CanonicalScalar has an arm for
  }
}

} // namespace

int scan_distinct(const Table *t, const llkv_projection *projections, uint32_t n_projections, const llkv_filter *filters, uint32_t n_filters, const llkv_eval_op *ops,
                  uint32_t n_ops, const llkv_scan_options *options, const llkv_scan_order_term *order, uint32_t n_order, uint64_t offset, uint64_t limit,
                  llkv_on_batch on_batch, void *user, uint64_t *selected_rows, uint64_t *distinct_rows) {
  if (selected_rows) *selected_rows = 0;
  if (distinct_rows) *distinct_rows = 0;
  // refusals: before any device work
  if (!t || !on_batch) return set_error(LLKV_INVALID_ARGUMENT, "NULL argument: llkv_hip_scan_distinct needs a table and an on_batch callback");
  if (n_projections && !projections) return set_error(LLKV_INVALID_ARGUMENT, "NULL argument: " + std::to_string(n_projections) + " projections without a projection array");
  for (uint32_t i = 0; i < n_projections; ++i)
    if (projections[i].computed)
      return set_error(LLKV_UNSUPPORTED, "scan DISTINCT with a computed projection (projection " + std::to_string(i) + "): its cells exist only after the gather");
  if (t->world > 1) return set_error(LLKV_UNSUPPORTED, "scan DISTINCT over a sharded table (world " + std::to_string(t->world) + "): deduplicate each rank's rows and merge them in the binding");
  int rc;
  if (n_order && (rc = topn_refusals(options, n_projections, order, n_order, offset, limit, 1))) return rc;
  if ((rc = ensure_device())) return rc;
  LoweredPlan proj;
  std::string err;
  if ((rc = lower_projection(table_resolver(*t), projections, n_projections, &proj, &err))) return set_error(rc, err);
  for (uint32_t i = 0; i < n_projections; ++i) {
    const ColumnInfo &ci = t->cols.at(projections[i].field_id).info;
    if (ci.wide128) return set_error(LLKV_UNSUPPORTED, "scan DISTINCT of field " + std::to_string(ci.field_id) + ": a Decimal128 column staged beyond 64 bits");
  }
  std::string forced;
  if (const char *e = std::getenv("LLKV_HIP_DISTINCT_ROUTE")) forced = e;
  if (!forced.empty() && forced != "direct" && forced != "hash")
    return set_error(LLKV_INVALID_ARGUMENT, "LLKV_HIP_DISTINCT_ROUTE=" + forced + ": direct or hash");
  uint64_t hash_mask = ~0ull;
  if (const char *e = std::getenv("LLKV_HIP_DISTINCT_HASH_BITS")) {
    const unsigned long k = std::strtoul(e, nullptr, 10);
    if (k < 64) hash_mask = (1ull << k) - 1;
  }

  // the selection scan_stream makes, in its order
  PhaseTrace trace("[llkv scan_distinct] %-22s %9.3f ms\n", g_ctx.stream);
  std::vector<uint32_t> gathered;
  if (!(options && options->include_nulls))
    for (uint32_t i = 0; i < n_projections; ++i) gathered.push_back(projections[i].field_id);
  Selection sel;
  if ((rc = run_selection(t, filters, n_filters, ops, n_ops, &sel, gathered.data(), (uint32_t)gathered.size()))) return rc;
  const uint64_t n = sel.n;
  if (selected_rows) *selected_rows = n;
  if (n == 0) return LLKV_OK; // no row is canonicalised: no batch, whatever the column types
  if (n >= (1ull << 32)) return set_error(LLKV_UNSUPPORTED, "scan DISTINCT over 2^32 selected rows or more");
  for (uint32_t i = 0; i < n_projections; ++i) // the reference fails at the first row it canonicalises (canonical.rs:134-136)
    if (const char *name = type_name(t->cols.at(projections[i].field_id).info.dtype))
      return set_error(LLKV_INVALID_ARGUMENT, std::string("building canonical scalar is not supported for column type ") + name);
  if (options && options->order_enabled && (rc = sort_selection(t, options, &sel))) return rc;
  trace.mark("selection");

  // the key, and the route: direct when the statistics bound every column and the cells are few
  DistinctParams p;
  std::memset(&p, 0, sizeof p);
  p.dev = sel.d_dev;
  p.n = n;
  p.n_cols = (int32_t)n_projections;
  unsigned __int128 cells = 1;
  std::string why_not_direct;
  for (uint32_t i = 0; i < n_projections; ++i) {
    const DeviceColumn &c = t->cols.at(projections[i].field_id);
    unsigned __int128 card = 0;
    describe_column(c, &p.c[i], &card);
    if (!why_not_direct.empty()) continue;
    if (card == 0) {
      why_not_direct = "field " + std::to_string(c.info.field_id) + " has no bounded value range";
      continue;
    }
    p.c[i].card = (unsigned long long)std::min<unsigned __int128>(card, (unsigned __int128)UINT64_MAX);
    p.c[i].stride = (unsigned long long)cells;
    cells *= card + (p.c[i].valid ? 1 : 0);
    if (cells > kDirectMaxCells) why_not_direct = "the key takes more than " + std::to_string(kDirectMaxCells) + " cells";
  }
  if (n_projections == 0) why_not_direct = "no projected column";
  bool direct = why_not_direct.empty();
  if (forced == "direct" && !direct) return set_error(LLKV_UNSUPPORTED, "LLKV_HIP_DISTINCT_ROUTE=direct: the direct route does not admit this projection (" + why_not_direct + ")");
  // a table of more cells than the hash route's slots buys nothing for a small selection: filling and reading it is the cost
  if (direct && forced.empty() && (uint64_t)cells > std::max<uint64_t>(1u << 16, 4 * n)) direct = false;
  if (forced == "hash") direct = false;
  uint64_t n_table = direct ? (uint64_t)cells : 2;
  if (!direct)
    while (n_table < 2 * n) n_table <<= 1;

  hipStream_t s = g_ctx.stream;
  Scratch table, flags, offsets, scan_tmp, counters;
  if ((rc = table.alloc(n_table * 4)) || (rc = flags.alloc(n * 8)) || (rc = offsets.alloc(n * 8)) || (rc = counters.alloc(16))) return rc;
  // from here on the stream runs ahead of the host: everything is waited for before the buffers go back to their pools
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{s};
  unsigned long long *d_occupied = counters.as<unsigned long long>();
  uint32_t *d_error = counters.as<uint32_t>() + 2;
  HIP_TRY(hipMemsetAsync(table.p, 0xFF, n_table * 4, s));
  HIP_TRY(hipMemsetAsync(flags.p, 0, n * 8, s));
  HIP_TRY(hipMemsetAsync(counters.p, 0, 16, s));
  if (direct) hipLaunchKernelGGL(distinct_direct_insert, dim3(dist_grid(n)), dim3(kDistBlock), 0, s, p, table.as<uint32_t>(), n_table, d_error);
  else hipLaunchKernelGGL(distinct_hash_insert, dim3(dist_grid(n)), dim3(kDistBlock), 0, s, p, table.as<uint32_t>(), n_table - 1, hash_mask, d_error);
  HIP_TRY(hipGetLastError());
  trace.mark(direct ? "insert (direct)" : "insert (hash)");
  hipLaunchKernelGGL(distinct_mark, dim3(dist_grid(n_table)), dim3(kDistBlock), 0, s, (const uint32_t *)table.as<uint32_t>(), n_table, n, flags.as<uint64_t>(), d_occupied, d_error);
  HIP_TRY(hipGetLastError());
  if ((rc = exclusive_scan_u64(flags.as<uint64_t>(), offsets.as<uint64_t>(), n, scan_tmp, s))) return rc;
  uint64_t before_last = 0, last_flag = 0, occupied = 0;
  uint32_t error = 0;
  Readback rb;
  if ((rc = rb.add(&before_last, offsets.as<uint64_t>() + (n - 1), 8, s)) || (rc = rb.add(&last_flag, flags.as<uint64_t>() + (n - 1), 8, s)) ||
      (rc = rb.add(&occupied, d_occupied, 8, s)) || (rc = rb.add(&error, d_error, 4, s)) || (rc = rb.wait()))
    return rc;
  const uint64_t d = before_last + last_flag;
  if (error & kDistErrProbes) return set_error(LLKV_INTERNAL, "scan DISTINCT: a row found neither its class nor an empty slot in " + std::to_string(n_table) + " probes");
  if (error & kDistErrRange) return set_error(LLKV_INTERNAL, "scan DISTINCT: a cell lies outside its column's statistics (direct route)");
  if (error & kDistErrIndex) return set_error(LLKV_INTERNAL, "scan DISTINCT: the table holds an index outside the selection");
  if (occupied != d || d == 0 || d > n)
    return set_error(LLKV_INTERNAL, "scan DISTINCT: " + std::to_string(occupied) + " occupied cells name " + std::to_string(d) + " rows of " + std::to_string(n));
  if (distinct_rows) *distinct_rows = d;
  if (trace.on) std::fprintf(stderr, "[llkv scan_distinct] route %s, %llu cells, %llu selected rows, %llu distinct\n", direct ? "direct" : "hash", (unsigned long long)n_table,
                             (unsigned long long)n, (unsigned long long)d);

  Selection first; // the first occurrences, in selection order
  first.n = d;
  first.d_ids = (uint64_t *)scratch_alloc(d * 8);
  first.d_dev = (uint64_t *)scratch_alloc(d * 8);
  if (!first.d_ids || !first.d_dev) return set_error(LLKV_INTERNAL, "device scratch allocation failed");
  hipLaunchKernelGGL(distinct_compact, dim3((uint32_t)((n + kDistBlock - 1) / kDistBlock)), dim3(kDistBlock), 0, s, (const uint64_t *)flags.as<uint64_t>(),
                     (const uint64_t *)offsets.as<uint64_t>(), n, d, (const uint64_t *)sel.d_dev, (const uint64_t *)sel.d_ids, first.d_dev, first.d_ids);
  HIP_TRY(hipGetLastError());
  trace.mark("survivors");

  if (n_order) rc = topn_over_selection(t, proj, projections, options, order, n_order, offset, limit, first, on_batch, user);
  else {
    const uint64_t end = limit > UINT64_MAX - offset ? UINT64_MAX : offset + limit;
    if (options && options->include_row_ids && offset < d && (rc = selection_report_ids(t, &first))) return rc;
    rc = deliver_windows(t, proj, first, offset, end, options, on_batch, user);
  }
  trace.mark("delivery");
  return rc;
}

} // namespace llkv

extern "C" llkv_status llkv_hip_scan_distinct(const llkv_hip_table *table, const llkv_projection *projections, uint32_t n_projections, const llkv_filter *filters,
                                              uint32_t n_filters, const llkv_eval_op *ops, uint32_t n_ops, const llkv_scan_options *options,
                                              const llkv_scan_order_term *order, uint32_t n_order, uint64_t offset, uint64_t limit, llkv_on_batch on_batch, void *user,
                                              uint64_t *selected_rows, uint64_t *distinct_rows) {
  return (llkv_status)llkv::scan_distinct(reinterpret_cast<const llkv::Table *>(table), projections, n_projections, filters, n_filters, ops, n_ops, options, order, n_order,
                                          offset, limit, on_batch, user, selected_rows, distinct_rows);
}
